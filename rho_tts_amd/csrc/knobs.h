// The process-wide launch-plan switches (rt_debug_tune, include/rho_tts_amd_debug.h): ONE table.  From it come the declarations
// below, the definitions and the descriptor array rt_debug_tune walks (debug.hip); tests/test_tune_cpu.py reads it as text.
//
//   X(code_base, name, default, lo, hi, "what the values mean; what was measured")
//
// rt_debug_tune(code_base + v, 0) with lo <= v <= hi sets the switch to v; a code in no row's [code_base + lo, code_base + hi] is
// refused.  Rows in ascending code order.  The switches are plain global atomics that the launch code reads directly by name
// (relaxed); they are written by rt_debug_tune alone, under the exclusive lock (common.h).  Every accepted call advances
// g_tune_epoch, which the decode graphs' signature carries (generate.hip): no captured frame outlives a changed plan.
#pragma once
#include "common.h"

#define RT_KNOBS(X) \
    X(0, g_skinny_variant, 0, 0, 2, "legacy skinny GEMM: 0 k_gemm_skinny, 1 k_gemm_skinny2<.,4>, 2 k_gemm_skinny2<.,8>") \
    X(100, g_decode_col, 1, 0, 1, "0 legacy 9-launch split-K decode, 1 column-owner GEMM + fused attention (5 launches per layer)") \
    X(200, g_use_graph, 1, 0, 1, "0 eager decode frames, 1 replayed from captured hipGraphs") \
    X(300, g_pred_nt, 0, 0, 1, "predictor weights: 0 cacheable loads (Infinity-Cache resident across its 15 passes), 1 non-temporal") \
    X(400, g_decode_lanes, 1, 1, 8, "decode lanes: groups of items decoding concurrently on their own streams (rt_generate)") \
    X(500, g_col_split, 0, 0, 4, "sub-tile split of narrow decode GEMMs: 0 automatic (col_split_for), 1 / 2 / 4 forced") \
    X(600, g_tile96, 1, 0, 1, "1: 128x96 workgroup tiles for N = 96 / 192 (codec decoder), 0: always 128x128") \
    X(700, g_col_rows64, 1, 0, 1, "1: one 64-row decode GEMM launch for the predictor's two-position pass, 0: two 32-row launches") \
    X(800, g_fuse_sample_embed, 1, 0, 1, "1: sampler + next-input embedding in one launch (predictor groups), 0: separate k_embed_rowsq") \
    X(900, g_prefill_fill, 3, 0, 99, "workgroups per CU a prefill GEMM's split-K aims for") \
    X(1000, g_xcd_order, 1, 0, 1, "1: tiled GEMMs run a row tile's column tiles back to back on one XCD") \
    X(1100, g_final_conv, 1, 0, 1, "the codec decoder's last conv: 1 its own LDS-window kernel, 0 a one-column GEMM") \
    X(1200, g_conv_win, 1, 0, 1, "1: k>1 convs on operand planes keep their input window in LDS (k_conv_win), 0: per-tap kernel") \
    X(1300, g_sync_parts, 0, 0, 1, "1: rt_generate waits for the stream after every frame part (bounds the dispatches in flight; profiling aid)") \
    X(1400, g_eos_check_every, 8, 1, 99, "frames between two host looks at the device-side end-of-sequence flags (1 = every frame)") \
    X(1500, g_attn_mfma, 0, 0, 2, "the talker's shared-prefix decode attention: 0 vector unit, 1 / 2 matrix cores with four rows / one row per workgroup (attention_mfma.hip); 1 measured " \
        "16.6 us per launch against 13.3 us for the vector-unit kernel at batch 32 / 460 prefix rows, so off") \
    X(1600, g_col_split4, 0, 0, 1, "1: the automatic split may go to quarter tiles (N <= 1024 on 256 CUs); measured 1.4 ms/step slower than half tiles") \
    X(1700, g_handover_every, 4, 1, 99, "queued items (n_items > rows): frames between two looks at the flags + row hand-overs.  Measured on the 1.7B model, 512 / 64 ragged texts on 32 " \
        "rows: 2 -> 487 / 445, 3 -> 489 / 445, 4 -> 491 / 447, 6 -> 485 / 445, 8 -> 477 / 428, 12 -> 475 / 434 audio-s/s (a hand-over costs ~1.4 ms, a waiting row 0.13 ms per frame)") \
    X(1800, g_conv_tall, 1, 0, 2, "k>1 convs of the 96- / 192-channel stages: 0 128-row tiles, 1 256-row tiles for long inputs, 2 always") \
    X(1900, g_prefill_mid, 1, 0, 3, "prompt prefills of 65..1024 rows: 0 split-K tiled kernel, 1 k_gemm_mid (no split-K slabs), 2 / 3 force its 64 / 128 tiles") \
    X(2000, g_col_max_rows, 64, 1, 64, "batches of up to 64 rows decode on the column-owner path while they have at most this many rows (65..128 rows always do, and only while this stands at 64).  Above 32 the talker's GEMMs take 64 rows per launch and the predictor's " \
        "two-position first pass runs as two 64-row launches: 715 audio-s/s at batch 64 against 510 at batch 32 (1.7B, bench.py --batch 64) - every weight byte serves twice the rows for " \
        "~1.4x the launch time") \
    X(2100, g_fuse_conv, 1, 0, 1, "1: a 96-channel k>1 conv and the 1x1 conv behind its activation run as one launch (launch_conv_pair); 0 switches the 192-channel pairs off as well") \
    X(2200, g_prefill_attn_mfma, 1, 0, 1, "prompt attention behind a shared voice prefix: 0 vector unit, 1 matrix cores") \
    X(2300, g_col_rows16, 0, 0, 1, "1: decode GEMM launches of <= 16 rows take the 128-VGPR MT = 1 instantiation (two workgroups per CU: decode lanes)") \
    X(2400, g_col_silu_x, 1, 0, 1, "1: gate/up GEMMs whose pairs are 1.5x the CUs run as one round of 1.5-pair workgroups, 0: one pair per workgroup (1.5 rounds)") \
    X(2600, g_conv_unroll, 1, 0, 1, "1: k = 7 convs run the tap-unrolled instantiation of k_conv_win, 0: the generic tap loop") \
    X(2700, g_frame_inc_fold, 0, 0, 1, "1: frame += 1 by the last workgroup of the frame's talker-input launch, 0: k_frame_inc (the fold measured 1-1.8 ms per step SLOWER)") \
    X(2800, g_pair_attn, 1, 0, 1, "1: two-position decode passes append both positions inside the fused attention launch, 0: k_qkv_post + k_attention") \
    X(2900, g_c2w_lean, 1, 0, 1, "1: rt_code2wav drops the third unit's unread residual-stream store and the waveform copy (the last conv writes the caller's buffer)") \
    X(3000, g_fuse_conv192, 1, 0, 1, "1: the 192-channel conv pairs fuse as well, weight fragments staged through LDS") \
    X(3100, g_pred_qkv_table, 1, 0, 1, "predictor passes 2..G-1: 1 layer 0's q/k/v row of the drawn code is copied from the table rt_model_finalize builds (by the launch " \
        "that embeds the code), 0 the layer-0 qkv GEMM launch runs (same bits either way)") \
    X(3200, g_col_rows128, 1, 0, 1, "generations on 65..128 rows: 1 one 128-row decode GEMM launch per weight matrix (k_gemm_col MT = 8: the weights are streamed once), " \
        "0 two 64-row launches (same bits either way).  Measured (1.7B, profiles/r18_rows128.txt): bench.py --corpus 512 --batch 128 1014 audio-s/s with 1 against 887 with 0 (five alternating pairs; 824 on 64 rows); " \
        "per launch at 128 rows qkv 13.7 / 16.3 us, o 12.0 / 14.2, gate/up 20.9 / 27.4, down 27.3 / 29.7 (one launch / two)") \
    X(3300, g_stt_gather_ranged, 1, 0, 1, "speech-to-text under a prompt policy, the gather between beam steps: 1 the ranged form (generated positions only; the prefix " \
        "sits in both caches), 0 the uniform form over [0, longest prefix of the group + step) (same bits either way; profiles/r20_stt_prompt.txt)") \
    X(3400, g_rowsq_wide, 1, 0, 1, "RMSNorm sum-of-squares partials of the decode GEMMs, rows of n partials with n % 64 == 0 and n <= 256: 1 stored permuted (rowsq_slot) " \
        "and fetched by the row-scale prologue in 2 / 4 16-byte requests per lane, 0 stored plainly and fetched in 16 dword requests (same bits either way; " \
        "profiles/r21_gemm_col_prologue.txt)") \
    X(3500, g_col_chunk_fit, 1, 0, 1, "STORE / RESID decode GEMM launches of up to 32 rows: 1 the chunk length follows the wave's run of k-tiles (one chunk of 4 for K <= 1024, " \
        "two of 6 for K = 3072: no clamped re-loads of the run's last tile), 0 chunks of 8 (same bits either way; profiles/r21_gemm_col_prologue.txt)") \
    X(3600, g_col_row_blocks, 2, 0, 2, "decode GEMM launches whose workgroups fill at most half of the CUs (the predictor's o / down / mtp: 128 on 256) deal their rows over " \
        "gridDim.y: 0 never, 1 launches of 33..64 rows as two 32-row blocks, 2 also launches of 17..32 rows as two 16-row blocks (same bits either way; " \
        "profiles/r24_row_blocks.txt)") \
    X(3700, g_col_tile_blocks, 2, 0, 2, "STORE / RESID decode GEMM launches at split 2 whose half-tile workgroups fill more than half of the CUs (the 1.7B talker's o / down, the " \
        "predictor's head: N = 2048, 256 workgroups of 32 rows x 8 columns) run whole-tile workgroups with their rows dealt over gridDim.y - as many workgroups, fewer bytes into " \
        "each CU's L1: 0 never, 1 launches of 33..64 rows as 32-row blocks, 2 also launches of 17..32 rows as 16-row blocks (same bits either way, the rowsq row keeps its " \
        "split-2 layout; profiles/r25_tile_blocks.txt)")

// The one switch set by rt_debug_tune's SECOND argument: applied when the code is 0..2 and the argument lies in lo..hi.
#define RT_KNOB_ARG(X) \
    X(0, g_skinny_waves_per_cu, 4, 1, 0x7fffffff, "legacy skinny GEMM: split-K is chosen so that about this many waves per CU stream weights")

#define RT_KNOB_EXTERN(base, name, def, lo, hi, doc) extern rt_knob name;
RT_KNOBS(RT_KNOB_EXTERN)
RT_KNOB_ARG(RT_KNOB_EXTERN)
#undef RT_KNOB_EXTERN
extern std::atomic<int> g_tune_epoch;       // accepted rt_debug_tune calls so far
