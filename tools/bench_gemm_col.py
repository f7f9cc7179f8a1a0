#!/usr/bin/env python3
"""Microbenchmark of the column-owner decode GEMM (back-to-back launches, HBM-cold weights)."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa
from rho_tts_amd import _native
ctx = _native.Context(0)
lib = ctx.lib
lib.rt_bench_gemm_col.argtypes = [C.c_void_p] + [C.c_int32] * 7 + [C.POINTER(C.c_double), C.POINTER(C.c_int64)]
shapes = [(32, 4096, 2048, 1, 0, "talker qkv  NORM STORE"), (32, 2048, 2048, 0, 1, "talker o    RESID"), (32, 12288, 2048, 1, 2, "talker gu   NORM SILU"),
          (32, 2048, 6144, 0, 1, "talker down RESID"), (32, 3072, 2048, 1, 0, "talker head NORM STORE"), (32, 4096, 1024, 1, 0, "pred qkv    NORM STORE"),
          (32, 1024, 2048, 0, 1, "pred o      RESID"), (32, 6144, 1024, 1, 2, "pred gu     NORM SILU"), (32, 1024, 3072, 0, 1, "pred down   RESID"),
          (32, 2048, 1024, 1, 0, "pred head   NORM STORE"), (32, 4096, 2048, 0, 0, "qkv plain STORE"), (8, 4096, 2048, 1, 0, "qkv M=8 NORM")]
if len(sys.argv) > 1 and sys.argv[1] == "hot":      # same matrix every launch, cacheable loads: L2 / Infinity-Cache resident weights
    for M, N, K, norm, epi, name in shapes:
        mb = N * K * 2 / 1e6
        us = C.c_double()
        st = (C.c_int64 * 8)()
        rc = lib.rt_bench_gemm_col(ctx.handle, M, N, K, norm | 2, epi, 1, 400, C.byref(us), st)
        ph = " ".join(f"{(st[i + 1] - st[i]) * 0.01:.2f}" for i in range(5))
        print(f"{name:26s} {mb:6.1f} MB  HOT {us.value:7.2f} us [{ph}]", flush=True)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "rows128":  # 128 rows: one MT = 8 launch (3201) against the two 64-row launches it replaces (3200)
    import statistics
    for M, N, K, norm, epi, name in [s for s in shapes[:4]]:
        mb = N * K * 2 / 1e6
        n_mats = max(2, int(600 / mb) + 1)
        t = {3201: [], 3200: []}
        for _ in range(5):                          # alternating pairs
            for code in (3201, 3200):
                lib.rt_debug_tune(code, 0)
                us = C.c_double()
                rc = lib.rt_bench_gemm_col(ctx.handle, 128, N, K, norm, epi, n_mats, 400, C.byref(us), None)
                assert rc == 0, rc
                t[code].append(us.value)
        lib.rt_debug_tune(3201, 0)
        us = C.c_double()
        assert lib.rt_bench_gemm_col(ctx.handle, 64, N, K, norm, epi, n_mats, 400, C.byref(us), None) == 0
        line = "   ".join(f"{label} {statistics.median(v):7.2f} us (min {min(v):.2f} max {max(v):.2f}) {mb / statistics.median(v):5.2f} TB/s"
                          for label, v in (("one 128-row launch", t[3201]), ("two 64-row launches", t[3200])))
        print(f"{name:26s} {mb:6.1f} MB  M=128  {line}   [one 64-row launch {us.value:7.2f} us]", flush=True)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "prologue":
    # what a launch does before its weight stream starts: the row-scale partials' layout (3400/3401) and the chunk length (3500/3501),
    # at 32 and 64 rows; in-kernel stamps 0 -> 1 (requests issued, row scales summed) and 0 -> 5 (whole workgroup 0).
    # `prologue plain`: no switch is touched (a build without them), one column
    import statistics
    plain = len(sys.argv) > 2 and sys.argv[2] == "plain"
    for M in (32, 64):
        for _, N, K, norm, epi, name in shapes[:10]:
            mb = N * K * 2 / 1e6
            n_mats = max(2, int(600 / mb) + 1)
            cols = []
            for wide in ((0,) if plain else (0, 1)):
                for fit in ((0,) if plain else (0, 1)):
                    if not plain:
                        assert lib.rt_debug_tune(3400 + wide, 0) == 0 and lib.rt_debug_tune(3500 + fit, 0) == 0
                    t, s01, s05 = [], [], []
                    for _ in range(3):
                        us = C.c_double()
                        st = (C.c_int64 * 8)()
                        assert lib.rt_bench_gemm_col(ctx.handle, M, N, K, norm, epi, n_mats, 300, C.byref(us), st) == 0
                        t.append(us.value); s01.append((st[1] - st[0]) * 0.01); s05.append((st[5] - st[0]) * 0.01)
                    cols.append(f"{'plain' if plain else f'wide {wide} fit {fit}'}: {statistics.median(t):6.2f} us (min {min(t):.2f}) 0>1 {statistics.median(s01):.2f} 0>5 {statistics.median(s05):.2f}")
            print(f"M={M:2d} {name:24s} " + " | ".join(cols), flush=True)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "rows":
    # the narrow predictor launches (N = 1024: 128 workgroups on 256 CUs) by row count, cacheable weights cycling through 32 matrices
    # (what the predictor's Infinity-Cache resident weights are to its 15 passes); median of three runs of 300 launches.
    # `rows`: no switch is touched (a build without 3600); `rows blocks`: one column per value of 3600 / 3601 / 3602
    import statistics
    codes = (3600, 3601, 3602) if len(sys.argv) > 2 and sys.argv[2] == "blocks" else (None,)
    for N, K, norm, epi, name in ((1024, 2048, 0, 1, "pred o    RESID"), (1024, 3072, 0, 1, "pred down RESID"), (1024, 2048, 1, 0, "pred mtp  NORM STORE")):
        for M in (16, 32, 64):
            cols = []
            for code in codes:
                if code is not None:
                    assert lib.rt_debug_tune(code, 0) == 0
                t = []
                for _ in range(3):
                    us = C.c_double()
                    assert lib.rt_bench_gemm_col(ctx.handle, M, N, K, norm | 2, epi, 32, 300, C.byref(us), None) == 0
                    t.append(us.value)
                cols.append(f"{'' if code is None else str(code) + ': '}{statistics.median(t):6.2f} us (min {min(t):.2f} max {max(t):.2f})")
            print(f"{name:22s} M={M:2d}  " + " | ".join(cols), flush=True)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "tiles":
    # the N = 2048 launches whose 256 half-tile workgroups (32 rows x 8 columns) become 256 whole-tile workgroups of half the rows
    # (16 x 16; 64 rows: 64 x 8 -> 32 x 16), HBM-cold with non-temporal and with cacheable weight loads; median of three runs of 300.
    # `tiles`: one column per value of 3700 / 3701 / 3702; `tiles plain`: no switch is touched (a build without 3700)
    import statistics
    codes = (None,) if len(sys.argv) > 2 and sys.argv[2] == "plain" else (3700, 3701, 3702)
    for N, K, norm, epi, name in ((2048, 2048, 0, 1, "talker o    RESID"), (2048, 6144, 0, 1, "talker down RESID"), (2048, 1024, 1, 0, "pred head   NORM STORE")):
        mb = N * K * 2 / 1e6
        n_mats = max(2, int(600 / mb) + 1)
        for M in (16, 32, 64):
            for cache, label in ((0, "non-temporal"), (2, "cacheable   ")):
                cols = []
                for code in codes:
                    if code is not None:
                        assert lib.rt_debug_tune(code, 0) == 0
                    t = []
                    for _ in range(3):
                        us = C.c_double()
                        assert lib.rt_bench_gemm_col(ctx.handle, M, N, K, norm | cache, epi, n_mats, 300, C.byref(us), None) == 0
                        t.append(us.value)
                    cols.append(f"{'' if code is None else str(code) + ': '}{statistics.median(t):6.2f} us (min {min(t):.2f} max {max(t):.2f})")
                print(f"{name:24s} M={M:2d} {label}  " + " | ".join(cols), flush=True)
    sys.exit(0)
for M, N, K, norm, epi, name in shapes:
    mb = N * K * 2 / 1e6
    n_mats = max(2, int(600 / mb) + 1)
    res = []
    for code in (501, 500):             # forced unsplit, automatic sub-tile split
        lib.rt_debug_tune(code, 0)
        us = C.c_double()
        st = (C.c_int64 * 8)()
        rc = lib.rt_bench_gemm_col(ctx.handle, M, N, K, norm, epi, n_mats, 400, C.byref(us), st)
        ph = " ".join(f"{(st[i + 1] - st[i]) * 0.01:.2f}" for i in range(5))
        res.append(f"{us.value:7.2f} us {mb / us.value:5.2f} TB/s (rc {rc}) [issue, first chunk, rest, reduce, epilogue: {ph}]")
    print(f"{name:26s} {mb:6.1f} MB  unsplit {res[0]}   auto split {res[1]}", flush=True)
