/*
 * rho_tts_amd_debug.h - measurement and test entry points of librho_tts_amd.so.
 *
 * NOT part of the drop-in boundary: nothing here stands behind an interface of the reference (rho-tts has no profiling, tuning or
 * kernel-test surface: SURVEY.md section 5), and a host binding of the generation path (rho_tts_amd.h) never
 * calls it.  Used by bench.py (rt_profile_*: the roofline figure), tests/ (rt_debug_*: single kernels against the CPU oracle)
 * and tools/ (rt_bench_*: microbenchmarks; rt_debug_tune: A/B switches).
 *
 * Threading: rt_debug_tune changes PROCESS-WIDE launch-plan switches.  It takes every context's work to a stop first - it waits
 * until no library call is executing on any context (calls hold a shared lock, the switch an exclusive one) and refuses
 * (RT_ERR_STATE) while a generation is in flight between rt_generate_begin and rt_generate_end on any model - so a thread that
 * tunes can never change the launch plan of a call or of a resumable generation that another thread has under way.
 */
#ifndef RHO_TTS_AMD_DEBUG_H
#define RHO_TTS_AMD_DEBUG_H

#include "rho_tts_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-kernel timing of the decode step for bench.py's roofline figure: when enabled, every weight-streaming GEMM
 * launch is bracketed by HIP events on the context's stream. */
RT_API int rt_profile_enable(rt_model* m, int32_t on);
RT_API int rt_profile_read(rt_model* m, int64_t* n_launches, double* total_ms, double* total_bytes);
/* The same sums over the recorded launches of ONE class of weight stream: 0 = talker layers, codec head, mtp projection (cross
 * HBM once per frame); 1 = the predictor's first pass over its layers + its heads (each byte's first use in the frame);
 * 2 = predictor passes 2.. over the same layers (re-streamed from the Infinity Cache).  SURVEY.md 8d counts classes 0 + 1. */
RT_API int rt_profile_read_class(rt_model* m, int32_t cls, int64_t* n_launches, double* total_ms, double* total_bytes);

/* ------------------------------------------------------------------ kernel-level test hooks
 * Exercise single kernels against a float32 reference (tests/test_kernels_gpu.py).  All pointers are HBM.
 * rt_debug_gemm: out[M][N] (f32) = A . W^T for a row-major bf16 W[N][K=taps*cin]; A is the implicit-GEMM view
 * of a channels-last activation [batch][rows_in][cin] (bf16; f32 when a_is_f32 = 1; f32 fed as hi+lo bf16 planes
 * when a_is_f32 = 2; a_is_f32 = 3: d_a holds the bf16 hi plane followed by the bf16 lo plane, as a producing epilogue
 * writes them): output row (b, t) reads input
 * rows t + tap_offset + tap*tap_stride, zero outside [0, rows_in).  mode 0: LDS-tiled kernel (split_k slabs are
 * summed on return), mode 1: weight-streaming skinny kernel (plain A only, M <= 64), mode 2: the prompt-prefill kernel
 * (k_gemm_mid: plain bf16 A, 65..1024 rows, K a multiple of 64, final sums from 64 x 64 tiles over the whole K). */
RT_API int rt_debug_gemm(rt_ctx* ctx, const void* d_a, int32_t a_is_f32, int64_t M, int32_t cin, int32_t taps, int32_t tap_stride,
                         int32_t tap_offset, int32_t rows_out, int32_t rows_in, const void* d_w_bf16, int32_t N,
                         const float* d_bias, int32_t act, float* d_out, int32_t mode, int32_t split_k);
/* q [M][heads][d] f32, caches [slots][kv_heads][max_pos][d] bf16 -> out [M][heads*d] bf16 */
RT_API int rt_debug_attention(rt_ctx* ctx, const float* d_q, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim,
                              const int32_t* d_row_slot, const int32_t* d_row_pos, int32_t window, const void* d_k, const void* d_v,
                              int32_t slots, int32_t max_pos, void* d_out_bf16);
/* The same attention over a cache held as hi + lo bf16 planes (value = hi + lo), float32 output - the form of the codec
 * pre-transformer and the audio-encoder transformer: q [M][heads][d] f32, each of d_k_hi / d_k_lo / d_v_hi / d_v_lo
 * [slots][kv_heads][max_pos][d] bf16 -> out [M][heads*d] f32. */
RT_API int rt_debug_attention_planes(rt_ctx* ctx, const float* d_q, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim,
                                     const int32_t* d_row_slot, const int32_t* d_row_pos, int32_t window, const void* d_k_hi,
                                     const void* d_k_lo, const void* d_v_hi, const void* d_v_lo, int32_t slots, int32_t max_pos,
                                     float* d_out_f32);
/* The dominant decode kernel on its own (gemm_col.hip k_gemm_col; launched as model_stack.hip launches it: row blocks of <= 64, or ONE launch of 65..128 rows unless rt_debug_tune(3200),
 * production sub-tile split when split = 0).  Row-major operands; the hook converts to / from the fragment-tiled layout (x, next and
 * act in buffers as wide as N rounded up to whole 32-column k-tiles, so that any N is a valid width).
 *   A [M][K] bf16, W [N][K] bf16 (epi 2: gate rows [0, N/2) then up rows), M <= 128, K % 32 == 0, row_off % 16 == 0
 *   d_rowsq [M][rowsq_n] or NULL: partial sums of squares of the pre-norm row; acc rows are scaled by rsqrt(sum/K + eps)
 *   epi 0 STORE: d_x [M][N] f32 out = scale_row * (A W^T) + bias
 *   epi 1 RESID: d_x [M][N] f32 in/out: x += scale .* (scale_row * (A W^T) + bias); d_next_bf16 [M][N] = bf16(next_norm_w .* x);
 *                d_rowsq_out [M][ceil(N/16)*split] partial sums of squares of the new x
 *   epi 2 SILU : d_act_bf16 [M][N/2] = bf16(silu(g) * u)
 * nt: 1 = non-temporal weight loads (talker), 0 = cacheable (predictor). */
RT_API int rt_debug_gemm_col(rt_ctx* ctx, const void* d_a_bf16, int32_t M, int32_t K, const void* d_w_bf16, int32_t N, int32_t epi, int32_t split,
                             int32_t row_off, int32_t nt, const float* d_rowsq, int32_t rowsq_n, float eps, const float* d_bias,
                             const float* d_scale, float* d_x, const float* d_next_norm_w, void* d_next_bf16, float* d_rowsq_out,
                             void* d_act_bf16);
/* The decode step's fused attention launch: qkv [M][(heads+2kv)*d] f32 (raw projections), q/k norm weights [d] or NULL,
 * cos/sin [max_pos][d/2]; row r is sequence slot row_slot[r] at position row_pos[r] + pos_add: its K/V row is appended to the
 * caches [slots][kv_heads][max_pos][d] bf16, then it attends to positions [0, pos]; positions < prefix_len are read from
 * prefix_slot (-1: no shared prefix).  out [M][heads*d] bf16 row-major.  d_row_slot NULL: row r is slot r; d_row_pos NULL: every
 * row at pos_add (the array-free form of the residual-code predictor's passes). */
RT_API int rt_debug_attention_fused(rt_ctx* ctx, const float* d_qkv, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim,
                                    const float* d_q_norm_w, const float* d_k_norm_w, float eps, const float* d_cos, const float* d_sin,
                                    const int32_t* d_row_slot, const int32_t* d_row_pos, int32_t pos_add, void* d_k, void* d_v,
                                    int32_t slots, int32_t max_pos, int32_t prefix_slot, int32_t prefix_len, void* d_out_bf16);
/* The same launch as a decode step of a multi-voice generation takes it (rt_generate_item_voices): the M rows are cut into 4-row
 * blocks, block b reads the prefix of voice h_block_voice[b] (host array, ceil(M / 4) entries), whose h_prefix_len[v] rows sit in
 * cache slot slots - n_voices + v.  Every block takes the form its voice takes alone: the matrix-core one (head_dim 128, 2 query
 * heads per kv head, >= 64 prefix rows; the call builds the tiles per voice) in one launch over those blocks, the vector one in a
 * second launch over the rows of the others.  d_row_slot / d_row_pos are required.  RT_ERR_INVALID before any launch: M outside
 * 1..128, n_voices outside 1..8, a block voice outside the voices, a prefix longer than max_pos. */
RT_API int rt_debug_attention_fused_voices(rt_ctx* ctx, const float* d_qkv, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim,
                                           const float* d_q_norm_w, const float* d_k_norm_w, float eps, const float* d_cos, const float* d_sin,
                                           const int32_t* d_row_slot, const int32_t* d_row_pos, int32_t pos_add, void* d_k, void* d_v,
                                           int32_t slots, int32_t max_pos, int32_t n_voices, const int32_t* h_prefix_len,
                                           const int32_t* h_block_voice, void* d_out_bf16);
/* The row plan of a multi-voice generation as host arithmetic (no GPU is touched).  Rows are cut into 4-row blocks and a block holds
 * rows of one voice: an item takes the lowest free row of a block of its voice, else the first row of the lowest block whose rows are
 * all free (the block is re-voiced), else it waits - and with it every later item of its voice; array order is kept within a voice.
 *   first != 0: the first wave of n_items items (h_voice[i] in 0..7) on at most max_rows (1..128) rows.  Outputs h_row_item [max_rows]
 *               (item on the row, -1 free), h_block_voice [ceil(max_rows / 4)] (-1: none), h_placed [n_items]; returns the run's rows:
 *               max_rows while items wait, else the last occupied row + 1.  One distinct voice gives item b on row b.
 *   first == 0: a hand-over on a run of max_rows rows: the three arrays hold the state (freed rows set to -1 by the caller) and are
 *               updated; returns the number of items placed.  h_revoiced (optional): blocks that changed from one voice to another.
 * A bad argument returns -1. */
RT_API int rt_debug_voice_row_plan(const int32_t* h_voice, int32_t n_items, int32_t max_rows, int32_t first, int32_t* h_row_item,
                                   int32_t* h_block_voice, int32_t* h_placed, int32_t* h_revoiced);
/* Prompt-prefill attention behind a shared prefix: q [M][heads][d] f32 (normed, roped), row r = sequence slot row_slot[r] at position
 * row_pos[r], whose K / V rows up to that position are already in the caches; positions < prefix_len are read from prefix_slot.
 * mode 0: the vector-unit kernel, 1: the matrix-core form the model uses for prompt rows (head_dim 128, 2 query heads per kv head,
 * prefix_len >= 64), 2: the prefix slot's OWN prefill - rows must be positions 0 .. M - 1 of prefix_slot (M >= 64), causal, the keys in
 * front of each 8-row block on the matrix cores.  out [M][heads*d] bf16. */
RT_API int rt_debug_attention_prefill(rt_ctx* ctx, const float* d_q, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim,
                                      const int32_t* d_row_slot, const int32_t* d_row_pos, const void* d_k, const void* d_v, int32_t slots,
                                      int32_t max_pos, int32_t prefix_slot, int32_t prefix_len, int32_t mode, void* d_out_bf16);
/* One draw per row: logits [M][V] f32 -> tokens [M].  item ids 0..M-1. */
RT_API int rt_debug_sample(rt_ctx* ctx, const float* d_logits, int32_t M, int32_t V, const rt_sampling* sp, uint64_t seed,
                           int32_t frame, int32_t group, int32_t suppress_from, int32_t allow_token, uint8_t* d_seen, int32_t* d_out);
/* The two stages of probabilistic YIN's back half on their own (tests/test_features_batch_gpu.py); the pitch model must be set
 * (rt_features_set_pitch_model).  HOST pointers on both sides; one stream synchronisation per call.
 * rt_debug_features_observe: h_cmnd [n_frames][n_lags] float64 -> h_log_obs [n_frames][2 n_bins] (definition: observation_log_probs
 *   of rho_tts_amd/features.py).
 * rt_debug_features_viterbi: h_log_obs = the log-obs of n_clips clips back to back, clip c with h_n_frames[c] rows of 2 n_bins
 *   -> h_states [n_clips][stride] int32, -1 behind a clip's last frame (definition: viterbi_banded; one workgroup per clip). */
RT_API int rt_debug_features_observe(rt_features* f, const double* h_cmnd, int32_t n_frames, int32_t n_lags, int32_t min_period,
                                     double* h_log_obs);
RT_API int rt_debug_features_viterbi(rt_features* f, const double* h_log_obs, const int32_t* h_n_frames, int32_t n_clips, int32_t* h_states,
                                     int32_t stride);

/* The stages of the speaker encoder on their own (tests/test_speaker_embed_gpu.py); the encoder must be finalized.  One stream
 * synchronisation per call.
 * rt_debug_spk_mel: one clip in HBM through the front end of rt_spk_embed_batch (resample, volume, optional trim with h_voice_flags
 *   [n_voice_flags], zero padding to the last partial's end) -> h_mel [frames][40] float32, frames = 1 + padded length / 160
 *   (RT_ERR_LENGTH above cap_frames), and h_n16 = the 16-kHz length after preprocessing, before the padding.
 * rt_debug_spk_lstm: h_partials [n_partials][160][40] float32 on the HOST -> h_embed [n_partials][256], the unit-norm embedding of
 *   every partial (three LSTM layers, projection, ReLU, norm). */
RT_API int rt_debug_spk_mel(rt_spk* s, const float* d_pcm, int64_t n_samples, int32_t sample_rate_in, const uint8_t* h_voice_flags,
                            int32_t n_voice_flags, float* h_mel, int32_t cap_frames, int32_t* h_n_frames, int64_t* h_n16);
RT_API int rt_debug_spk_lstm(rt_spk* s, const float* h_partials, int32_t n_partials, float* h_embed);

/* The speech-to-text path below the ids with more than one row (tests/test_stt_batch_gpu.py): the first window of n_clips clips (at
 * most one group, 32) through the front end and encoder -> d_states [n_clips][n_ctx][d_model] float32 in HBM.  Clip i's states
 * among the n_clips rows are, bit for bit, what rt_stt_encode gives for that window as the only row (the first chunk_seconds of the
 * clip, cut as rt_stt_transcribe cuts it). */
RT_API int rt_debug_stt_encode_batch(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips, int32_t sample_rate_in,
                                     float* d_states);

/* The two kernels of the beam path on their own (tests/test_stt_beam_kernel_gpu.py).
 * rt_debug_stt_beam_step: one step of the rule on logits the caller supplies (HBM, float32, [n_windows * row_stride][cfg.vocab]; beam j
 *   of window w is row w * row_stride + j; row_stride is `beam`, or 1 for the step behind the prefix) with the handle's masks and
 *   end-of-sequence id.  In, per row w * beam + j: the beams' cumulative scores; per window: live beams, finished entries so far, done
 *   flag.  Out, per row: next token and parent ROW (-1 where the step wrote none), the new scores, the finished list's beams and
 *   scores (entry k of window w at w * beam + k; the entries from h_n_finished[w] on are this step's); per window: live beams, finished
 *   entries, done flag; and the number of windows still decoding.  n_windows * beam <= 32.
 * rt_debug_stt_beam_reorder: fills the four planes of a cache [layers][rows][heads][max_pos][head_dim] with the 16-bit pattern
 *   (i * 40503 + plane * 12289) & 0x7fff (i: the element's index in its plane) and those of a second one with 0xbeef, gathers row
 *   h_src[r]'s positions [0, len) into row r of the second, and returns all eight planes in h_planes. */
RT_API int rt_debug_stt_beam_step(rt_stt* s, const float* d_logits, int32_t row_stride, const float* h_scores_in, int32_t n_windows, int32_t beam,
                                  const int32_t* h_n_live, const int32_t* h_n_finished, const int32_t* h_done, int32_t first_step, int32_t step,
                                  int32_t* h_next_tok, int32_t* h_parent, float* h_scores_out, int32_t* h_n_live_out, int32_t* h_fin_beam,
                                  float* h_fin_score, int32_t* h_n_finished_out, int32_t* h_done_out, int32_t* h_live_windows);
RT_API int rt_debug_stt_beam_reorder(rt_ctx* ctx, int32_t layers, int32_t rows, int32_t heads, int32_t max_pos, int32_t head_dim, const int32_t* h_src,
                                     int32_t len, uint16_t* h_planes);
/* The kernels of a prompt policy on their own (rt_stt_set_prompt; tests/test_stt_prompt_kernel_gpu.py).
 * rt_debug_stt_beam_reorder_range: rt_debug_stt_beam_reorder with a range per row - row h_src[r]'s positions [h_lo[r], h_hi[r]),
 *   0 <= lo <= hi <= max_pos, go into row r of the second cache; everything else of it keeps the sentinel.
 * rt_debug_stt_prompt_prefix: the ragged prefix pass.  The first window of n_windows clips (1 .. 32) goes through the front end and
 *   the encoder; window w then decodes the h_len[w] tokens it is given (h_tokens: the windows' tokens one after the other, each an id
 *   of the vocabulary; 1 .. min(n_text_ctx / 2 + n_prefix - 1, n_text_ctx - 1) per window) at positions 0 .. h_len[w] - 1 of a cache
 *   slot of its own, all windows' rows in ONE pass, and d_logits [n_windows][vocab] (HBM, float32) receives the logits of every
 *   window's last row.  A window's logits do not depend on what it shares the pass with. */
RT_API int rt_debug_stt_beam_reorder_range(rt_ctx* ctx, int32_t layers, int32_t rows, int32_t heads, int32_t max_pos, int32_t head_dim, const int32_t* h_src,
                                           const int32_t* h_lo, const int32_t* h_hi, uint16_t* h_planes);
RT_API int rt_debug_stt_prompt_prefix(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_windows, int32_t sample_rate_in,
                                      const int32_t* h_tokens, const int32_t* h_len, float* d_logits);
/* rt_debug_stt_beam_step under the timestamp rule (tests/test_stt_seek_kernel_gpu.py; a handle with rt_stt_set_timestamps): the step
 * as rt_stt_transcribe_seek launches it.  Further in, per row: the history state - h_ts_flags_in bit 0: the row's last generated
 * token is a timestamp, bit 1: the one before it is (or the history holds fewer than two tokens); h_ts_last_in: the last timestamp
 * id of the row's history, 0: none - and max_initial_timestamp_index (-1: no limit; it binds when first_step is set).  Further out:
 * the state of every next beam, derived from its parent row's. */
RT_API int rt_debug_stt_beam_step_ts(rt_stt* s, const float* d_logits, int32_t row_stride, const float* h_scores_in, int32_t n_windows, int32_t beam,
                                     const int32_t* h_n_live, const int32_t* h_n_finished, const int32_t* h_done, int32_t first_step, int32_t step,
                                     int32_t max_initial_timestamp_index, const int32_t* h_ts_flags_in, const int32_t* h_ts_last_in,
                                     int32_t* h_next_tok, int32_t* h_parent, float* h_scores_out, int32_t* h_n_live_out, int32_t* h_fin_beam,
                                     float* h_fin_score, int32_t* h_n_finished_out, int32_t* h_done_out, int32_t* h_live_windows,
                                     int32_t* h_ts_flags_out, int32_t* h_ts_last_out);

/* One sampled step of the temperature fallback (k_stt_sample_select; tests/test_stt_sample_kernel_gpu.py) on logits the caller
 * supplies, shaped like rt_debug_stt_beam_step: n_rows rows (1 .. 8192, a multiple of `samples`, 1 .. 8), row r = sample r % samples
 * of window r / samples; logits in HBM, float32: [n_rows][cfg.vocab] for row_stride == samples, one row per WINDOW
 * ([n_rows / samples][cfg.vocab], the step behind the prefix) for row_stride == 1.  In: the temperature (> 0), the seed, the
 * temperature's index in its policy, per row the window key and the sample index (a row's pick depends on these, the step and its
 * logits alone), the rows' cumulative scores and done flags.  Out, per row: the pick (-1 for a row that came in done: such a row
 * comes back as it went in), the new score, the winning perturbed value x / T + g, the done flag; and the rows still decoding.
 * The book is allocated for the call, so the handle's decoder side does not grow with n_rows.
 * _ts (a handle with rt_stt_set_timestamps): the timestamp instantiation, with the rows' history state in and out as
 * rt_debug_stt_beam_step_ts. */
RT_API int rt_debug_stt_sample_step(rt_stt* s, const float* d_logits, int32_t row_stride, int32_t n_rows, int32_t samples, float temperature, uint64_t seed,
                                    int32_t temperature_index, const int32_t* h_key, const int32_t* h_sample, const float* h_scores_in, const int32_t* h_done,
                                    int32_t first_step, int32_t step, int32_t* h_next_tok, float* h_scores_out, float* h_win_val, int32_t* h_done_out,
                                    int32_t* h_live_rows);
RT_API int rt_debug_stt_sample_step_ts(rt_stt* s, const float* d_logits, int32_t row_stride, int32_t n_rows, int32_t samples, float temperature, uint64_t seed,
                                       int32_t temperature_index, const int32_t* h_key, const int32_t* h_sample, const float* h_scores_in, const int32_t* h_done,
                                       int32_t first_step, int32_t step, int32_t max_initial_timestamp_index, const int32_t* h_ts_flags_in,
                                       const int32_t* h_ts_last_in, int32_t* h_next_tok, float* h_scores_out, float* h_win_val, int32_t* h_done_out,
                                       int32_t* h_live_rows, int32_t* h_ts_flags_out, int32_t* h_ts_last_out);

/* k_stt_probe on logits the caller supplies (tests/test_stt_lang_kernel_gpu.py): n_rows (1 .. 32) rows of cfg.vocab float32 in HBM,
 * row r at d_logits + r * row_stride (row_stride >= cfg.vocab), with the handle's languages and no-speech id (rt_stt_set_languages)
 * -> per row the language id, its probability among the configured ids, and the no-speech probability. */
RT_API int rt_debug_stt_probe(rt_stt* s, const float* d_logits, int64_t row_stride, int32_t n_rows, int32_t* h_lang, float* h_lang_prob,
                              float* h_no_speech);

/* The kernels of rt_stt_align one at a time (tests/test_stt_align_gpu.py; csrc/stt_align.hip).  d_ pointers are HBM, h_ host memory.
 * rt_debug_stt_align_probs: k_stt_align_probs on q [q_rows][heads * head_dim] (float32) and one layer of a cross-attention cache the
 *   caller supplies as planes d_k_hi / d_k_lo (bf16 bits, [slots][heads][n_ctx][head_dim]; d_k_lo may be null): alignment row a reads row
 *   h_src[a] of q over slot h_slot[a] and writes t < h_frames[a]; the n_heads heads h_heads[] are written in that order to
 *   d_W [n_heads][n_rows][ldw] (ldw >= every h_frames[a]; cells that are not written keep the caller's bytes).
 * rt_debug_stt_align_matrix: k_stt_align_stats + k_stt_align_matrix on d_W [n_heads][n][F] -> d_M [n][F].
 * rt_debug_stt_dtw: k_stt_dtw on d_M [n][F] -> h_frames [n]; trace_mode -1: the trace in LDS when it fits, 0: in global memory,
 *   1: in LDS (RT_ERR_INVALID when it does not fit).
 * rt_debug_stt_align_stages: one group (1 .. 32 windows, every one with ids) of a real rt_stt_align call, arguments as there, and
 *   beside its outputs the call's W as [n_windows][n_heads][h_shape[0]][h_shape[1]] (zero where nothing is written: rows >= n + 1,
 *   t >= F of the window) in h_W and its M, window by window [n + 1][F], in h_M (capacities in floats; RT_ERR_LENGTH with h_shape set
 *   when one is short). */
RT_API int rt_debug_stt_align_probs(rt_ctx* ctx, const float* d_q, int32_t q_rows, int32_t heads, int32_t head_dim, const uint16_t* d_k_hi, const uint16_t* d_k_lo,
                                    int32_t slots, int32_t n_ctx, const int32_t* h_src, const int32_t* h_slot, const int32_t* h_frames, int32_t n_rows,
                                    const int32_t* h_heads, int32_t n_heads, int32_t ldw, float* d_W);
RT_API int rt_debug_stt_align_matrix(rt_ctx* ctx, const float* d_W, int32_t n_heads, int32_t n, int32_t F, int32_t median_width, float* d_M);
RT_API int rt_debug_stt_dtw(rt_ctx* ctx, const float* d_M, int32_t n, int32_t F, int32_t trace_mode, int32_t* h_frames);
/* Events around the launches rt_stt_align adds to a decoder pass (tools/bench_stt_align.py): returns the milliseconds summed since the
 * last call - the capture launches, statistics + matrix, the paths - clears the sums and switches the recording on or off. */
RT_API int rt_debug_stt_align_timing(rt_stt* s, int32_t on, double* ms_capture, double* ms_matrix, double* ms_dtw);
RT_API int rt_debug_stt_align_stages(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_windows, int32_t sample_rate_in,
                                     const int32_t* h_text_ids, const int32_t* h_text_offsets, const int32_t* h_language, float* h_W, int64_t w_cap, float* h_M,
                                     int64_t m_cap, int32_t* h_shape, int32_t* h_token_frame, float* h_token_logprob);

/* ------------------------------------------------------------------ row kernels on their own (tests/test_rowops_gpu.py)
 * Each hook checks its arguments, calls the production launch_* function of rowops.hip (so the launcher's dispatch and its refusals
 * are under test too), synchronises the stream and returns the status.  All pointers are HBM unless named h_*; matrices are
 * row-major on both sides.  Kernels that write the fragment-tiled layout (common.h tile_off) are run on tiled copies that the hook
 * makes FROM the caller's row-major output buffers and copies back, so whatever the kernel leaves alone keeps the caller's bytes;
 * with raw_tiled = 1 the caller's buffers ARE the tiled ones (16 * ceil(rows / 16) rows of H) and nothing is converted. */

/* launch_add_rmsnorm: x [M][H] += scale .* (sum of n_slabs slabs [n_slabs][M][H] + slab_bias) in place (n_slabs > 0), then
 * rmsnorm(x) .* w -> out_bf16 / out_f32 [M][H] (either may be NULL; w == NULL: the update alone).  slab_bias, scale [H] optional. */
RT_API int rt_debug_add_rmsnorm(rt_ctx* ctx, float* d_x, int32_t M, int32_t H, const float* d_slabs, int32_t n_slabs, const float* d_slab_bias,
                                const float* d_scale, const float* d_w, float eps, void* d_out_bf16, float* d_out_f32);
/* launch_rowsq: block i reads row src_rows[i] (default i; entries in [0, M)) of x [M][H], or - from block g_first on, when g_table
 * is set - row g_idx[frame * g_idx_frame_stride + (i - g_first) * g_idx_stride] of the f32 table (a negative index is a row of
 * zeros; frame = *g_frame_ptr or 0), and writes output row dst_rows[i] (default i; entries in [0, out_rows)):
 * rowsq [out_rows][rowsq_n] = (sum of squares, 0, ...), x_out [out_rows][H] f32 (optional), a_out [out_rows][H] = bf16(norm_w .* x)
 * (optional, needs norm_w).  H % 32 == 0 with a tiled output, H % 4 == 0 otherwise. */
RT_API int rt_debug_rowsq(rt_ctx* ctx, const float* d_x, int32_t M, int32_t H, float* d_rowsq, int32_t rowsq_n, float* d_x_out, void* d_a_out_bf16,
                          const float* d_norm_w, const int32_t* d_src_rows, const int32_t* d_dst_rows, int32_t out_rows, const float* d_g_table,
                          const int32_t* d_g_idx, int32_t g_idx_stride, int32_t g_first, const int32_t* d_g_frame_ptr, int64_t g_idx_frame_stride,
                          int32_t raw_tiled);
/* launch_norm_tiled_rows: out [M][H] = w .* x * rsqrt(sum(rowsq[row][0 .. rowsq_n)) / H + eps); x [M][H] row-major (the hook tiles it). */
RT_API int rt_debug_norm_tiled_rows(rt_ctx* ctx, const float* d_x, const float* d_rowsq, int32_t rowsq_n, const float* d_w, float eps, int32_t M,
                                    int32_t H, float* d_out);
/* launch_embed_rowsq: row r = add_vec + sum_j table_j[idx[r * idx_stride + j]] over n_src bf16 tables (h_tables: HOST array of
 * device pointers, h_row_strides: HOST array of row strides in elements; a negative index skips the source), or + row
 * idx[r * idx_stride] of f32_table [.][H]; idx is moved by *frame_ptr * idx_frame_stride.  Out: x_out [M][H] f32, a_out [M][H] =
 * bf16(norm_w .* x), rowsq [M][rowsq_n].  frame_inc (== frame_ptr) + arrive (a zeroed counter): the launch also adds 1 to the frame
 * counter.  qkv_table [.][qkv_n] f32: row idx[r * idx_stride] (negative: row 0) is copied to qkv_out [M][qkv_n]. */
RT_API int rt_debug_embed_rowsq(rt_ctx* ctx, const void* const* h_tables, const int64_t* h_row_strides, int32_t n_src, const float* d_f32_table,
                                const int32_t* d_idx, int32_t idx_stride, const int32_t* d_frame_ptr, int64_t idx_frame_stride, int32_t M, int32_t H,
                                const float* d_add_vec, float* d_rowsq, int32_t rowsq_n, float* d_x_out, void* d_a_out_bf16, const float* d_norm_w,
                                int32_t* d_frame_inc, uint32_t* d_arrive, const float* d_qkv_table, float* d_qkv_out, int32_t qkv_n,
                                int32_t raw_tiled);
/* launch_silu_mul: slabs [n_slabs][M][2 I] (gate columns, then up) -> silu(sum gate) * (sum up) as out_f32 [M][I] if given, else out_bf16.
 * launch_reduce_slabs: out [M][N] = act(bias + sum of slabs [n_slabs][M][N]), act in {0 none, 1 SiLU, 2 GELU}, to f32 and / or bf16.
 * launch_f32_to_bf16: n elements, round to nearest even. */
RT_API int rt_debug_silu_mul(rt_ctx* ctx, const float* d_slabs, int32_t n_slabs, int32_t M, int32_t I, void* d_out_bf16, float* d_out_f32);
RT_API int rt_debug_reduce_slabs(rt_ctx* ctx, const float* d_slabs, int32_t n_slabs, int64_t M, int32_t N, const float* d_bias, int32_t act,
                                 float* d_out_f32, void* d_out_bf16);
RT_API int rt_debug_f32_to_bf16(rt_ctx* ctx, const float* d_x, int64_t n, void* d_out_bf16);
/* launch_qkv_post: slabs [n_slabs][M][(heads + 2 kv_heads) * d] -> q_out [M][heads][d] f32 (RMSNorm with q_norm_w [d] unless NULL,
 * rotate-half RoPE with cos / sin [max_pos][d / 2] unless NULL), k / v rows to the caches [slots][kv_heads][max_pos][d] bf16 at
 * (row_slot[r], row_pos[r] + pos_add + *frame_ptr); k_lo / v_lo (both or neither): the low planes.  The hook reads row_slot /
 * row_pos back and refuses a row outside the caches. */
RT_API int rt_debug_qkv_post(rt_ctx* ctx, const float* d_slabs, int32_t n_slabs, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim,
                             const float* d_q_norm_w, const float* d_k_norm_w, float eps, const float* d_cos, const float* d_sin,
                             const int32_t* d_row_slot, const int32_t* d_row_pos, int32_t pos_add, float* d_q_out, void* d_k, void* d_v,
                             void* d_k_lo, void* d_v_lo, int32_t slots, int32_t max_pos, const int32_t* d_frame_ptr);
/* launch_gather_sum: out [M][H] = add_vec + add_rows[add_row_idx[r] (default r; negative: none)] + sum_j table_j[idx[r * idx_stride + j]]
 * (tables as in rt_debug_embed_rowsq; idx_stride 0 = n_src).  launch_gather_f32: out [M][H] = table[idx[r * idx_stride]], zeros for a
 * negative index.  Both move idx by *frame_ptr * idx_frame_stride and write f32 and / or bf16. */
RT_API int rt_debug_gather_sum(rt_ctx* ctx, const void* const* h_tables, const int64_t* h_row_strides, int32_t n_src, const int32_t* d_idx, int32_t M,
                               int32_t H, const float* d_add_vec, const float* d_add_rows, const int32_t* d_add_row_idx, float* d_out_f32,
                               void* d_out_bf16, int32_t idx_stride, const int32_t* d_frame_ptr, int64_t idx_frame_stride);
RT_API int rt_debug_gather_f32(rt_ctx* ctx, const float* d_table, int32_t H, const int32_t* d_idx, int32_t M, float* d_out_f32, void* d_out_bf16,
                               int32_t idx_stride, const int32_t* d_frame_ptr, int64_t idx_frame_stride);
/* launch_dwconv_ln: x [B][T][C] f32 -> LayerNorm over C (ln_w, ln_b, eps) of the causal depthwise conv (w [7][C], b [C]) -> out [B][T][C].
 * launch_code_embed_mean: out [rows][H] = mean over q of table [Q][codebook][H] (bf16) at codes [rows][Q], codes clamped to the codebook.
 * launch_final_conv: hi / lo bf16 planes [B][T][C], w [7][C], bias [1] -> wav [b * wav_stride + t] = clamp(conv, -1, 1). */
RT_API int rt_debug_dwconv_ln(rt_ctx* ctx, const float* d_x, int32_t B, int32_t T, int32_t C, const float* d_w, const float* d_b, const float* d_ln_w,
                              const float* d_ln_b, float eps, float* d_out);
RT_API int rt_debug_code_embed_mean(rt_ctx* ctx, const void* d_table_bf16, int32_t codebook, int32_t Q, int32_t H, const int32_t* d_codes, int64_t rows,
                                    float* d_out);
RT_API int rt_debug_final_conv(rt_ctx* ctx, const void* d_hi, const void* d_lo, int32_t B, int32_t T, int32_t C, const float* d_w, const float* d_bias,
                               float* d_wav, int64_t wav_stride);

/* rt_debug_gemm's tiled mode (mode 0, split_k 1) with the whole epilogue exposed (tests/test_gemm_epilogue_gpu.py): every field of
 * the launch's GemmEpi - out = act(acc + bias) * scale + residual (the residual may be out_f32 itself), to f32 / bf16 / hi + lo
 * planes; out2 = act2(out) (3 SnakeBeta with snake2_a / snake2_ib, 5 ELU) to the same kinds; all outputs [M][ldc], ldc >= N (0 = N).
 * act: 0 none, 1 SiLU, 2 GELU, 3 SnakeBeta (snake_a, snake_ib), 4 clamp to [-1, 1], 5 ELU.  a_form as rt_debug_gemm's a_is_f32.
 * d_w2_bf16 [N][N] + e2 (optional): the 1x1 conv behind this conv's SnakeBeta in the same launch, launch_gemm(..., w2, e2).
 * pair_mode 1 asks conv_pair_fusable first, as the codec decoder does, and returns RT_ERR_UNSUPPORTED where it declines; 2 goes
 * to launch_gemm directly, whose own refusal is then the status. */
typedef struct rt_debug_epi {
    const float* bias;
    const float* scale;
    const float* residual;
    float* out_f32;
    void* out_bf16;
    void* out_hi;
    void* out_lo;
    const float* snake_a;
    const float* snake_ib;
    float* out2_f32;
    void* out2_bf16;
    void* out2_hi;
    void* out2_lo;
    const float* snake2_a;
    const float* snake2_ib;
    int64_t ldc;
    int32_t act;
    int32_t act2;
} rt_debug_epi;
RT_API int rt_debug_gemm_epi(rt_ctx* ctx, const void* d_a, int32_t a_form, int64_t M, int32_t cin, int32_t taps, int32_t tap_stride, int32_t tap_offset,
                             int32_t rows_out, int32_t rows_in, const void* d_w_bf16, int32_t N, const rt_debug_epi* e, const void* d_w2_bf16,
                             const rt_debug_epi* e2, int32_t pair_mode);

/* The sampler launch in the form the decode loop gives it (generate.hip, rt_gen_run::enqueue_a; tests/test_sampler_frame_gpu.py):
 * every caller-visible field of SampleArgs (kernels.h).  The hook calls launch_sample - its dispatch and refusals are under test -
 * synchronises once and returns the status.
 *   logits [n_slabs][M][V] f32, summed in slab order; item_ids [M] (the low half keys the random stream); *seed and *frame are read
 *   on the device; row r draws at its own frame *frame - frame_off[r] (frame_off NULL: 0) in code group `group`; the end of sequence
 *   (eos_token, -1: none) is admitted for a row when eos_live != 0 and its own frame >= min_frames, tokens >= suppress_from are
 *   forbidden otherwise; seen [M][V] (optional) is the penalty history, read and updated; forced (optional) [frames][forced_fs]:
 *   row r takes forced[*frame * forced_fs + r] when that is >= 0.
 *   Outputs of frame f = *frame: out[f * out_fs + r * out_stride] = the token (0 for an end of sequence),
 *   eos_flag[f * eos_fs + r] (optional), logits_copy[f * copy_fs + r * V + i] = the summed logits (optional).
 *   emb_table [V][emb_H] f32 (optional; V <= 4096, emb_H % 32 == 0): the drawn token's row becomes emb_x [M][emb_H] f32, emb_a [M][emb_H]
 *   = bf16(emb_norm_w .* x) and emb_rowsq [M][emb_rowsq_n] = (sum of squares, 0, ...); with emb_qkv_table [V][emb_qkv_n] f32 its row of the
 *   token is copied to emb_qkv_out [M][emb_qkv_n] and only emb_x is written.  emb_x / emb_a are row-major here: the kernel runs on
 *   tiled copies made from them and copied back (see the row-kernel hooks above).
 * Refused before any launch: a NULL ctx / args / logits / item_ids / seed / frame / out, M < 1, V < 1, n_slabs < 1, out_stride < 1,
 * *frame < 0, a frame_off entry above *frame, and - with an embedding - a forced token >= V. */
typedef struct rt_debug_sample_frame_args {
    const float* d_logits;
    const int64_t* d_item_ids;
    const uint64_t* d_seed;
    const int32_t* d_frame;
    const int32_t* d_frame_off;
    uint8_t* d_seen;
    const int32_t* d_forced;
    int32_t* d_out;
    int32_t* d_eos_flag;
    float* d_logits_copy;
    const float* d_emb_table;
    const float* d_emb_norm_w;
    float* d_emb_rowsq;
    float* d_emb_x;
    void* d_emb_a_bf16;
    const float* d_emb_qkv_table;
    float* d_emb_qkv_out;
    int64_t out_fs, eos_fs, forced_fs, copy_fs;
    rt_sampling sp;
    int32_t n_slabs, M, V;
    int32_t suppress_from, group;
    int32_t eos_token, eos_live, min_frames;
    int32_t out_stride;
    int32_t emb_H, emb_rowsq_n, emb_qkv_n;
} rt_debug_sample_frame_args;
RT_API int rt_debug_sample_frame(rt_ctx* ctx, const rt_debug_sample_frame_args* args);

/* ------------------------------------------------------------------ the conditioning front-end's own kernels (encoder.hip;
 * tests/test_encoder_kernels_gpu.py).  Each hook checks its pointers, calls the production launch_* function (whose dispatch and
 * refusals are under test too), synchronises the stream once and returns the status.  All pointers are HBM unless named h_*.
 *
 * launch_enc_conv0: pcm [T] -> x [T][C] f32 = bias[c] + sum_k w[c][k] * pcm[t - (K - 1) + k] (zeros in front of the clip; K = the number
 *   of taps), hi / lo [T][C] = the bf16 operand planes of ELU(x).  C must divide 256.  T = 0 launches nothing.
 * launch_rvq: the split residual vector quantiser.  sem, aco [T][D]; h_cbT: HOST array of Q device pointers to the TRANSPOSED
 *   codebooks [D][K] (K entries, K <= 4096; D <= 4096; Q >= 1) -> codes [T][Q]: level 0 quantises sem, levels 1 .. Q - 1 quantise aco
 *   residually; distances in float32, ascending d, one rounding per operation; the lowest index wins a tie; a row no entry wins
 *   (a non-finite vector) gets code 0.  d_aco is IN/OUT: on return it holds the residual after the last acoustic level
 *   (aco - sum of the chosen entries of levels 1 .. Q - 1, subtracted in that order in float32); with Q == 1 it is unchanged.
 *   T = 0 launches nothing.
 * launch_stats_pool: x [T][C] -> out [2 C] = (mean over t, sqrt(variance about that mean + 1e-5)), T >= 1.
 * launch_gemv_f32: y [N] = W [N][K] . x [K] + b (b may be NULL), then max(., 0) when relu is set. */
RT_API int rt_debug_enc_conv0(rt_ctx* ctx, const float* d_pcm, int64_t T, int32_t C, int32_t K, const float* d_w, const float* d_bias, float* d_x,
                              void* d_hi, void* d_lo);
RT_API int rt_debug_rvq(rt_ctx* ctx, const float* d_sem, float* d_aco, int32_t T, int32_t D, int32_t K, int32_t Q, const void* const* h_cbT,
                        int32_t* d_codes);
RT_API int rt_debug_stats_pool(rt_ctx* ctx, const float* d_x, int32_t T, int32_t C, float* d_out);
RT_API int rt_debug_gemv_f32(rt_ctx* ctx, const float* d_W, const float* d_b_or_NULL, const float* d_x, int32_t N, int32_t K, int32_t relu,
                             float* d_y);
/* rt_voice_encode (same launches, same codes and speaker vector) that additionally copies the intermediates oracle/encoder.py names
 * to HOST buffers, each optional: feats, tf [2 F][enc.tf.hidden] (conv features; transformer output), emb [F][enc.tf.hidden] (after
 * the stride-2 conv), sem, aco [F][enc.vq_dim] (the quantiser's inputs, before it runs), F = *h_n_frames. */
RT_API int rt_debug_voice_encode_stages(rt_model* m, const float* h_pcm, int64_t n_samples, int32_t max_frames, float* h_feats, float* h_tf,
                                        float* h_emb, float* h_sem, float* h_aco, int32_t* h_codes, int32_t* h_n_frames,
                                        float* h_speaker_embed);

/* A/B switches for measurements and tests (process-wide; the defaults are the fast path).  One row per switch, as in the table
 * they are generated from (rho_tts_amd/csrc/knobs.h: defaults, accepted ranges, measurement notes).  A code that no row accepts is
 * refused with RT_ERR_INVALID and changes nothing.  `code`:
 *   0..2 legacy skinny-GEMM variant (`arg` > 0: its waves per CU; `arg` is ignored by every other code)
 *   100/101 legacy 9-launch / column-owner decode
 *   200/201 eager / hipGraph frames
 *   300/301 predictor weights cacheable / non-temporal
 *   400 + n: n decode lanes (n = 1..8)
 *   500 automatic, 501/502/504 forced sub-tile split of narrow decode GEMMs
 *   600/601 128x96 codec tiles off/on
 *   700/701 32-row / 64-row decode GEMM launches
 *   800/801 separate / fused sampler + next-input embedding
 *   900 + n: prefill split-K target of n workgroups per CU (n = 0..99, default 3)
 *   1000/1001 XCD-aware tile order of the tiled GEMM off/on
 *   1100/1101 the codec decoder's last conv as a one-column GEMM / in its own kernel
 *   1200/1201 k>1 convs on operand planes on the per-tap kernel / with their input window in LDS
 *   1300/1301 stream sync after every decode frame part off/on (bounds the dispatches in flight under rocprofv3 --pmc)
 *   1400 + n: end-of-sequence flags fetched every n frames (n = 1..99, default 8; 1401 = a copy + wait per frame)
 *   1500/1501/1502 shared-prefix decode attention on the vector unit / on the matrix cores with four rows / one row per workgroup
 *   1600/1601 quarter-tile split off/on
 *   1700 + n: queued items (rt_generate with n_items > max_batch) take over finished rows every n frames (n = 1..99, default 4)
 *   1800/1801/1802 narrow-channel (96 / 192) k>1 convs on 128-row tiles / 256-row tiles for long inputs / 256-row tiles always
 *   1900/1901/1902/1903 prompt-prefill GEMMs on the split-K tiled kernel / on k_gemm_mid (automatic, 64 x 64, 128 x 128 tiles)
 *   2000 + n: batches of up to n rows (n = 1..64, default 64) decode on the column-owner path, larger ones of <= 64 rows on the legacy
 *        split-K path (65..128 rows decode on the column-owner path alone, and only while n stands at 64)
 *   2100/2101 the codec decoder's 96-channel residual units as two launches (k = 7 conv, 1x1 conv) / one fused launch
 *   2200/2201 prompt-prefill attention behind a shared voice prefix on the vector unit / on the matrix cores
 *   2300/2301 decode GEMMs of <= 16 rows on the 32-row / the two-workgroups-per-CU 16-row instantiation
 *   2400/2401 gate/up decode GEMM whose tile pairs are 1.5x the CUs: one pair per workgroup (1.5 rounds) / 1.5 pairs per workgroup (one round)
 *   2600/2601 the codec decoder's k = 7 convs on the generic / the tap-unrolled instantiation of k_conv_win
 *   2700/2701 the decode frame counter advanced by a launch of its own / by the last workgroup of the frame's talker-input launch
 *   2800/2801 the predictor's two-position first pass: q/k norm + RoPE + append as a launch of its own in front of the attention / inside the fused attention
 *   2900/2901 rt_code2wav with / without the residual-stream store of every stage's third unit (no reader) and the waveform copy behind the last conv
 *   3000/3001 the codec decoder's 192-channel residual units as two launches / one fused launch (k = 7 with tap unrolling; 2100 switches both widths off)
 *   3100/3101 predictor passes 2..G-1: layer 0's qkv GEMM launch / its q/k/v row copied from the per-code table built by rt_model_finalize
 *   3200/3201 generations on 65..128 rows: two 64-row decode GEMM launches per weight matrix / one 128-row launch (same bits)
 *   3300/3301 speech-to-text under a prompt policy, the cache gather between beam steps: positions [0, longest prefix + step) of every row / each row's generated positions only (same bits)
 *   3400/3401 the decode GEMMs' RMSNorm sum-of-squares partials (rows of n partials, n % 64 == 0, n <= 256): stored plainly and fetched one dword per request / stored permuted and fetched 16 bytes per request (same bits)
 *   3500/3501 STORE / RESID decode GEMM launches of up to 32 rows: weight / activation chunks of 8 k-tiles / of the length of the wave's run (4 for K <= 1024, 6 for K = 3072; same bits)
 *   3600/3601/3602 decode GEMM launches whose workgroups fill at most half of the CUs: one workgroup per column tile for all rows / launches of 33..64 rows as two 32-row blocks / also launches of 17..32 rows as two 16-row blocks (same bits either way)
 *   3700/3701/3702 STORE / RESID decode GEMM launches at split 2 whose half-tile workgroups fill more than half of the CUs: half tiles for all rows / launches of 33..64 rows as whole tiles x two 32-row blocks / also launches of 17..32 rows as whole tiles x two 16-row blocks (same bits either way)
 * The rt_bench_* entry points are the microbenchmarks behind tools/bench_*.py (for rt_bench_gemm_col choose
 * n_mats * N * K * 2 bytes > 512 MB to stream from HBM, not from cache). */
RT_API int rt_debug_tune(int32_t code, int32_t arg);
/* The row-block rule of the column-owner decode GEMM's launcher as host arithmetic (no GPU is touched): the rows per block that a
 * launch of M rows, width N (gate + up for epi 2), epilogue epi and sub-tile split (<= 0: the automatic one) takes on a device of
 * n_cu compute units under the current switches (3600..3602), or 0 when one workgroup per column tile has all the rows.
 * A bad argument returns -1. */
RT_API int rt_debug_col_row_blocks(int32_t n_cu, int32_t M, int32_t N, int32_t epi, int32_t split);
/* The tile-block rule of the same launcher (3700..3702), same arguments: 16 / 32 when the launch runs whole-tile workgroups with its
 * rows dealt over two blocks of that many rows while its rowsq row keeps the split-2 layout, or 0 (rt_debug_col_row_blocks answers
 * for the row-block rule alone, which comes first; the two never hold together).  A bad argument returns -1. */
RT_API int rt_debug_col_tile_blocks(int32_t n_cu, int32_t M, int32_t N, int32_t epi, int32_t split);
RT_API int rt_bench_gemm_col(rt_ctx* ctx, int32_t M, int32_t N, int32_t K, int32_t a_norm, int32_t epi, int32_t n_mats, int32_t iters,
                             double* avg_us, int64_t* stamps8);
/* The cache gather between two beam steps of the speech-to-text decoder on its own (tools/bench_stt_prompt.py): two caches of
 * [layers][rows][heads][max_pos][head_dim] x 4 planes, neighbouring rows swap; microseconds per launch (device events over `iters`
 * launches back to back) of the ranged form over positions [prefix, prefix + step) and of the uniform form over [0, prefix + step). */
RT_API int rt_bench_stt_gather(rt_ctx* ctx, int32_t layers, int32_t rows, int32_t heads, int32_t max_pos, int32_t head_dim, int32_t prefix, int32_t step,
                               int32_t iters, double* us_ranged, double* us_uniform);
RT_API int rt_bench_launch(rt_ctx* ctx, int32_t grid_wgs, int32_t n, int32_t use_graph, int32_t reps, double* us_per_launch);
RT_API int rt_bench_grid_barrier(rt_ctx* ctx, int32_t wgs, int32_t threads, int32_t n, int32_t mode, double* us_per_barrier, int32_t* aborted);
RT_API int rt_bench_sample(rt_ctx* ctx, const float* d_logits, int32_t M, int32_t V, const rt_sampling* sp, int32_t iters, double* avg_us,
                           int64_t* stamps8);
/* iters back-to-back launches of the decode step's fused attention: M rows at position prefix_len + own_len - 1, the first
 * prefix_len positions read from a shared prefix slot (shared = 1) or from each row's own slot (0), cycling through `layers`
 * cache regions; zeros as operands.  M <= 128; above 64 rows the launch is frame-indexed as a decode step's is, and shared | 2
 * runs the same rows as blocks of 64. */
/* The same launch single-voice against multi-voice (tools/bench_voices.py): M rows behind n_voices (1..8) prefixes of prefix_len rows
 * each; *us_single = every row behind voice 0 by the single-voice kernel, *us_multi = block b behind voice b % n_voices by the
 * multi-voice kernel reading the block table; the form (vector unit / matrix cores) is the one rt_debug_tune 1500 / 1501 selects for
 * both.  Two alternating passes of `iters` back-to-back launches each after a warm-up; microseconds per launch. */
RT_API int rt_bench_attention_fused_voices(rt_ctx* ctx, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim, int32_t prefix_len,
                                           int32_t own_len, int32_t n_voices, int32_t layers, int32_t iters, double* us_single, double* us_multi);
RT_API int rt_bench_attention_fused(rt_ctx* ctx, int32_t M, int32_t heads, int32_t kv_heads, int32_t head_dim, int32_t prefix_len, int32_t own_len,
                                    int32_t shared, int32_t layers, int32_t iters, double* avg_us);
RT_API int rt_bench_gemm_skinny(rt_ctx* ctx, int32_t M, int32_t N, int32_t K, int32_t split_k, int32_t n_mats, int32_t iters,
                                double* avg_us, int32_t* used_split);

#ifdef __cplusplus
}
#endif
#endif /* RHO_TTS_AMD_DEBUG_H */
