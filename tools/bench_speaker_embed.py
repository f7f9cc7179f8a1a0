#!/usr/bin/env python3
"""Speaker embeddings of one validation chunk (SpeakerEmbedder.batch -> rt_spk_embed_batch: one native call, one launch per stage,
three recurrent launches, one synchronisation) on seeded weights: 32 synthetic voiced clips of 4 s at 24 kHz, in HBM.

Reports, to stdout and to --out:
  * the time per chunk: a host clock around calls that end in the call's own stream synchronisation, after a warm-up, `--iters` calls
    per repeat, five repeats, the median and the spread;
  * the network alone on the same partials (rt_debug_spk_lstm: 3 recurrent launches + head, with its host-to-device copy of the
    partials), as a first bound on the recurrent share;
  * with --kernel-stats DIR (the output directory of a SEPARATE `rocprofv3 --kernel-trace --stats -d DIR -- python
    tools/bench_speaker_embed.py --iters 3 --no-cpu` run): the time of every k_spk_* kernel and the recurrent kernel's share of their sum;
  * for comparison the float32 torch.nn.LSTM + head on 16 CPU threads for the same partials (the oracle of tests/speaker_embed_ref.py
    in float32), and the chunk times on file for the other two stages of the validation loop.
No pass / fail: these are first measurements.
    python tools/bench_speaker_embed.py [--clips 32] [--seconds 4] [--iters 20] [--out FILE] [--kernel-stats DIR] [--no-cpu]"""
import argparse
import csv
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rho_tts_amd import _native
from rho_tts_amd import speaker as S

SR, REPEATS = 24000, 5
ON_FILE = ["drift features, same chunk shape: batch() 16.47 ms per chunk (profiles/r13_features_one_path.txt, median of run 1)",
           "speech-to-text, same chunk shape, 16 new tokens: greedy batch 57.50 ms, beam 5 173.02 ms per chunk (profiles/r11_stt_beam.txt)"]


def voiced(seconds, f0, seed):
    t = np.arange(int(seconds * SR)) / SR
    x = 0.3 * sum(np.sin(2 * np.pi * f0 * (k + 1) * t) / (k + 1) for k in range(5)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
    x[: int(0.1 * SR)] = 0.0
    return (x + 1e-3 * np.random.default_rng(seed).standard_normal(x.shape[0])).astype(np.float32)


def timed(fn, iters):
    """ms per call: `iters` calls per repeat (each ends in a stream synchronisation), REPEATS repeats."""
    out = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return sorted(out)


def kernel_stats(directory):
    """{kernel name: (calls, total ns)} of the k_spk_* rows of rocprofv3's kernel_stats.csv under `directory`."""
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Name", "")
                if "k_spk_" in name:
                    short = name[name.index("k_spk_"):].split("(")[0]             # demangled: up to the argument list
                    if name.startswith("_Z"):
                        short = short.split("E")[0]                               # mangled: up to the end of the nested name
                    calls, total = rows.get(short, (0, 0))
                    rows[short] = (calls + int(r["Calls"]), total + int(r["TotalDurationNs"]))
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ctx = _native.Context(0)
    emb = S.SpeakerEmbedder(ctx, synthetic=True)
    clips = [torch.from_numpy(voiced(a.seconds, 110.0 + 7.0 * c, c)).cuda() for c in range(a.clips)]
    torch.cuda.synchronize()
    e, parts = emb.batch_partials(clips, SR)                   # warm-up, and the shape of the work
    P = int(parts.sum())
    flop = 2.0 * P * S.PARTIAL_FRAMES * 4 * S.HIDDEN * ((S.N_MELS + S.HIDDEN) + 2 * (2 * S.HIDDEN))
    say(f"{a.clips} clips of {a.seconds:g} s at {SR} Hz: {P} partials of 160 frames ({int(parts.min())} .. {int(parts.max())} per clip), "
        f"{-(-P // 16)} tiles of 16; {3 * S.PARTIAL_FRAMES} dependent steps; {flop / 1e9:.1f} GFLOP in the three LSTM layers; "
        f"norms 1 within {float(np.abs(np.linalg.norm(e.astype(np.float64), axis=1) - 1).max()):.2g}")
    emb.batch(clips, SR)
    t = timed(lambda: emb.batch(clips, SR), a.iters)
    say(f"rt_spk_embed_batch, whole call: median {t[REPEATS // 2]:.3f} ms per chunk ({t[REPEATS // 2] / a.clips:.3f} ms per clip), "
        f"smallest {t[0]:.3f}, largest {t[-1]:.3f} over {REPEATS} repeats of {a.iters} calls")
    rng = np.random.default_rng(1)
    partials = rng.standard_normal((P, S.PARTIAL_FRAMES, S.N_MELS)).astype(np.float32)
    emb.debug_lstm(partials)
    tn = timed(lambda: emb.debug_lstm(partials), a.iters)
    say(f"rt_debug_spk_lstm on {P} partials (3 recurrent launches + head + a {partials.nbytes / 1e6:.1f} MB upload): median {tn[REPEATS // 2]:.3f} ms, "
        f"smallest {tn[0]:.3f}, largest {tn[-1]:.3f} = {100.0 * tn[REPEATS // 2] / t[REPEATS // 2]:.0f} % of the whole call's median")
    if a.kernel_stats:
        rows = kernel_stats(a.kernel_stats)
        total = sum(v[1] for v in rows.values())
        say(f"kernel times of a separate rocprofv3 --kernel-trace --stats run ({a.kernel_stats}):")
        for name, (calls, ns) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
            say(f"  {name:<28} {calls:6d} calls   {ns / max(calls, 1) / 1e3:10.1f} us per call   {100.0 * ns / max(total, 1):5.1f} % of the k_spk_* time")
        rec = sum(v[1] for k, v in rows.items() if "k_spk_lstm" in k)
        say(f"  recurrent kernel's share of the k_spk_* kernel time: {100.0 * rec / max(total, 1):.1f} %" if rows else "  no k_spk_* rows found")
    if not a.no_cpu:
        torch.set_num_threads(16)
        st = S.synthetic_state()
        net = torch.nn.LSTM(S.N_MELS, S.HIDDEN, num_layers=S.LAYERS, batch_first=True)
        net.load_state_dict({k[len("lstm."):]: torch.from_numpy(v) for k, v in st.items() if k.startswith("lstm.")})
        w, b = torch.from_numpy(st["linear.weight"]), torch.from_numpy(st["linear.bias"])
        x = torch.from_numpy(partials)

        def cpu():
            with torch.no_grad():
                _, (h, _) = net(x)
                v = torch.relu(h[-1] @ w.T + b)
                return v / v.norm(dim=1, keepdim=True)
        ref = cpu().numpy()
        got = emb.debug_lstm(partials)
        tc = []
        for _ in range(3):
            t0 = time.perf_counter()
            cpu()
            tc.append((time.perf_counter() - t0) * 1e3)
        say(f"float32 torch.nn.LSTM + head on {torch.get_num_threads()} CPU threads, same {P} partials: median {sorted(tc)[1]:.1f} ms "
            f"(network only, no front end); max |device - torch float32| = {float(np.abs(got - ref).max()):.3g}")
    say("on file, for the other stages of the validation loop:")
    for s in ON_FILE:
        say("  " + s)
    emb.close()
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
