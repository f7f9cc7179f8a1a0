#!/usr/bin/env python3
"""Where one batched transcription goes, from a rocprofv3 kernel trace of `python tools/bench_stt.py --once`: the kernels from the
first group launch of the front end (k_resample_group / k_logmel_frames_group) to the end of the trace, split into front end,
encoder GEMMs, encoder attention, other encoder kernels and the decoder (everything from the first k_stt_embed on), with the idle
time between kernels (host gaps: launches, the per-step read of the live count) of the encoder and decoder phases.
usage: stt_trace_split.py <dir-or-csv>"""
import csv, os, sys


def find(path):
    if os.path.isfile(path):
        return path
    for root, _, files in os.walk(path):
        for f in files:
            if f.endswith("kernel_trace.csv"):
                return os.path.join(root, f)
    raise SystemExit("no kernel_trace.csv under " + path)


rows = []
with open(find(sys.argv[1])) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Kernel_Name") or ""))
rows.sort()
first = next((i for i, r in enumerate(rows) if "_group" in r[2]), None)
if first is None:
    raise SystemExit("no batched front-end kernel in the trace")
rows = rows[first:]
embed = next((i for i, r in enumerate(rows) if "k_stt_embed" in r[2]), len(rows))
busy = {"front end": 0, "encoder GEMMs": 0, "encoder attention": 0, "encoder other": 0, "decoder kernels": 0}
calls = dict.fromkeys(busy, 0)
for i, (s, e, n) in enumerate(rows):
    if i >= embed:
        k = "decoder kernels"
    elif "k_resample" in n or "k_logmel" in n or "k_stt_fill" in n:
        k = "front end"
    elif "k_gemm_tiled" in n:
        k = "encoder GEMMs"
    elif "k_attention" in n:
        k = "encoder attention"
    else:
        k = "encoder other"
    busy[k] += e - s
    calls[k] += 1
span = rows[-1][1] - rows[0][0]
enc_span = (rows[embed][0] if embed < len(rows) else rows[-1][1]) - rows[0][0]
dec_span = span - enc_span
enc_busy = sum(v for k, v in busy.items() if k != "decoder kernels")
print(f"one batched call, first group kernel to last kernel: {span / 1e6:.2f} ms, {len(rows)} kernels")
for k, v in busy.items():
    print(f"  {k:18s} {v / 1e6:8.2f} ms  {100.0 * v / span:5.1f} %  {calls[k]:5d} launches")
print(f"  {'gaps, encoder phase':18s} {(enc_span - enc_busy) / 1e6:8.2f} ms  {100.0 * (enc_span - enc_busy) / span:5.1f} %")
print(f"  {'gaps, decoder phase':18s} {(dec_span - busy['decoder kernels']) / 1e6:8.2f} ms  {100.0 * (dec_span - busy['decoder kernels']) / span:5.1f} %")
