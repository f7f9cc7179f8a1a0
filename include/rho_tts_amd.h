/*
 * rho_tts_amd.h — C ABI of the MI355X-native generation path for rho-tts.
 *
 * Everything a host binds is declared here: extern "C", plain pointers and
 * sizes, no torch / C++ types.  The reference (rhofield/rho-tts v1.1.4) is pure
 * Python and has no FFI of its own; each entry point therefore cites the
 * reference *Python* interface it stands behind (paths relative to
 * /root/reference/src/rho_tts/).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every function returns an rt_status (0 = ok); rt_last_error(ctx) holds text
 *   - "d_" parameters are device (HBM) pointers, "h_" parameters host pointers
 *   - all device work is issued on the context's stream (rt_set_stream lets a
 *     host share its own, e.g. torch's current stream)
 *   - the library is callable from any host thread; calls on one context are
 *     serialised by an internal mutex (base_tts.py has no re-entrancy guard and
 *     the UI shares one instance across threads, ui/state.py:54,85-87)
 *
 * Status -> Python exception mapping used by the provider
 * (base_tts.py:786-797 decides retry vs. propagate on exactly these classes):
 *   RT_ERR_INVALID   -> ValueError                  (configuration error, never retried)
 *   RT_ERR_OOM       -> RuntimeError("out of memory ...")   (empty_cache + retry)
 *   RT_ERR_LENGTH    -> RuntimeError("length ...")          (retry)
 *   RT_ERR_CANCELLED -> CancelledException          (cancellation.py:14)
 *   anything else    -> RuntimeError
 */
#ifndef RHO_TTS_AMD_H
#define RHO_TTS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_API __attribute__((visibility("default")))

#define RT_ABI_VERSION 6

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID = 1,
    RT_ERR_OOM = 2,
    RT_ERR_LENGTH = 3,
    RT_ERR_HIP = 4,
    RT_ERR_CANCELLED = 5,
    RT_ERR_STATE = 6,
    RT_ERR_UNSUPPORTED = 7
} rt_status;

typedef struct rt_ctx rt_ctx;     /* one per (process, GPU) */
typedef struct rt_model rt_model; /* weights + KV cache + workspaces of one Qwen3-TTS-shaped model */

/* ------------------------------------------------------------------ context */

RT_API int rt_abi_version(void);
RT_API const char* rt_status_string(int status);
/* device_ordinal: HIP device index (LOCAL_RANK in a one-process-per-GPU job). */
RT_API int rt_create(int device_ordinal, rt_ctx** out_ctx);
RT_API int rt_destroy(rt_ctx* ctx);
RT_API const char* rt_last_error(rt_ctx* ctx);
/* hip_stream: a hipStream_t (NULL restores the context's own stream). */
RT_API int rt_set_stream(rt_ctx* ctx, void* hip_stream);
RT_API int rt_synchronize(rt_ctx* ctx);
/* Name of the GPU architecture the context runs on, e.g. "gfx950". */
RT_API int rt_device_info(rt_ctx* ctx, char* arch, size_t arch_cap, int* n_cu, int64_t* hbm_free, int64_t* hbm_total);

/* --------------------------------------------------------- post-processing
 * One fused launch, one workgroup per text item, standing behind the numeric
 * leaves of the pipeline:
 *   _trim_silence          base_tts.py:348-392      RT_POST_TRIM_START / _END
 *   _remove_dc_offset      base_tts.py:394-399      RT_POST_DC
 *   _apply_fades           base_tts.py:401-433      RT_POST_FADE_IN / _OUT
 *   _smooth_segment_join   base_tts.py:435-536      RT_POST_JOIN (implies per-position trim flags)
 *   QwenTTS._post_process_audio + _apply_windowed_normalization
 *                          providers/qwen.py:268-378  RT_POST_LOUDNESS
 *   _validate_sound_decay  base_tts.py:297-323      RT_POST_DECAY (statistics only)
 * The full per-item tail of _run_pipeline (base_tts.py:912-926) is
 * RT_POST_PIPELINE.
 */
#define RT_POST_TRIM_START 0x01u
#define RT_POST_TRIM_END   0x02u
#define RT_POST_DC         0x04u
#define RT_POST_FADE_IN    0x08u
#define RT_POST_FADE_OUT   0x10u
#define RT_POST_JOIN       0x20u
#define RT_POST_LOUDNESS   0x40u
#define RT_POST_DECAY      0x80u
#define RT_POST_PIPELINE   (RT_POST_TRIM_START | RT_POST_TRIM_END | RT_POST_DC | RT_POST_FADE_IN | \
                            RT_POST_FADE_OUT | RT_POST_JOIN | RT_POST_LOUDNESS | RT_POST_DECAY)

typedef struct rt_post_params {
    int32_t sample_rate;        /* BaseTTS.sample_rate                                   */
    float   silence_threshold;  /* 10^(silence_threshold_db/20), base_tts.py:367         */
    int32_t window;             /* int(sr*0.01)                base_tts.py:366           */
    int32_t fade;               /* int(sr*fade_duration_sec)   base_tts.py:420           */
    int32_t crossfade;          /* int(sr*crossfade_duration_sec) base_tts.py:455        */
    int32_t pause;              /* int(sr*inter_sentence_pause_sec) base_tts.py:519; 0 = none */
    int32_t loud_window;        /* int(sr*2.0)                 qwen.py:293               */
    int32_t trim_enabled;       /* BaseTTS.trim_silence                                  */
    double  target_rms_db;      /* -23.0   qwen.py:278                                   */
    double  max_gain_db;        /* 18.0    qwen.py:280                                   */
    double  max_amplitude;      /* 0.95    qwen.py:309                                   */
    double  decay_threshold;    /* BaseTTS.sound_decay_threshold                         */
    uint32_t stages;            /* RT_POST_* mask                                        */
    uint32_t reserved;
} rt_post_params;

typedef struct rt_post_stats {
    int64_t out_len;            /* samples written for the item                           */
    int64_t first_trim_start;   /* trim bounds of the item's first segment (leaf calls)   */
    int64_t first_trim_end;
    double  decay_ratio;        /* last-third RMS / first-third RMS (1.0 on the guards)   */
    double  rms_out;            /* RMS of the written samples                             */
    int32_t decay_ok;
    int32_t all_silent;         /* every segment was below the silence threshold          */
    int32_t fallback_concat;    /* reference's "direct concatenation" path was taken      */
    int32_t windowed_applied;   /* the 2-s windowed gain envelope was applied             */
} rt_post_stats;

/* Upper bound of the output length of an item (sum of segment lengths + pauses). */
RT_API int64_t rt_post_capacity(const rt_post_params* p, int32_t n_segments, const int64_t* h_seg_len);

/* Device-resident form: segment samples already in HBM (the vocoder's output).
 *   h_item_first_seg [n_items+1]  segments of item i are [first[i], first[i+1])
 *   h_seg_ptr        [n_seg]      device pointers to float32 samples
 *   h_seg_len        [n_seg]
 *   h_seg_trim       [n_seg] or NULL: per-segment RT_POST_TRIM_* override (ignored with RT_POST_JOIN
 *                    for items of >1 segment, where the position decides, base_tts.py:469-474)
 *   h_out_ptr        [n_items]    device pointers, capacity >= rt_post_capacity()
 *   h_stats          [n_items]    results (host)
 * Returns after the results are on the host. */
RT_API int rt_post_process(rt_ctx* ctx, const rt_post_params* p, int32_t n_items,
                           const int32_t* h_item_first_seg, const float* const* h_seg_ptr,
                           const int64_t* h_seg_len, const uint8_t* h_seg_trim,
                           float* const* h_out_ptr, const int64_t* h_out_cap, rt_post_stats* h_stats);

/* Host-buffer form (what the reference hands over: CPU float32 tensors, qwen.py:265).
 * Same arguments with host sample pointers; stages through HBM (PCIe-inclusive). */
RT_API int rt_post_process_host(rt_ctx* ctx, const rt_post_params* p, int32_t n_items,
                                const int32_t* h_item_first_seg, const float* const* h_seg_ptr,
                                const int64_t* h_seg_len, const uint8_t* h_seg_trim,
                                float* const* h_out_ptr, const int64_t* h_out_cap, rt_post_stats* h_stats);

/* float32 [-1,1] -> int16 PCM with the reference's truncating conversion (base_tts.py:664-666). */
RT_API int rt_pcm16(rt_ctx* ctx, const float* d_in, int64_t n, int16_t* d_out);

/* Sub-segment streaming (an EXTENSION - BaseTTS.stream yields whole segments, base_tts.py:1132-1190): the
 * per-segment leaves of stream() (base_tts.py:1170-1176: _post_process_audio, _trim_silence, _remove_dc_offset, _apply_fades)
 * for ONE chunk of a segment that is still being decoded.  The two segment-wide quantities are taken from the segment's first
 * chunk and carried: h_dc_gain[0] = DC offset, h_dc_gain[1] = linear gain to the target RMS (in/out).
 *   RT_STREAM_MEASURE     first chunk: measure gain (target RMS / RMS of the raw chunk's AUDIBLE span - first to last 10-ms frame above
 *                         the silence threshold - held to +-30 dB; over the WHOLE chunk, unclamped, when the chunk is also the last: a
 *                         segment handed over whole is levelled as the reference levels it) and dc (after the trim) and return
 *                         them; else apply as given.
 *                         A chunk with no audible frame measures nothing and returns gain 0: pass RT_STREAM_MEASURE (with the
 *                         first-chunk trim and fade flags) again with the next chunk and drop this one's output
 *   RT_STREAM_TRIM_START  drop leading silence (first chunk)     RT_STREAM_TRIM_END  drop trailing silence (last chunk)
 *   RT_STREAM_FADE_IN / _OUT  raised-cosine ramps of p->fade samples at the chunk's start / end (skipped below 2 x fade samples)
 * y = 0.95 tanh(x gain / 0.95) - dc; the 2-s windowed decay correction needs the whole segment and is not applied.
 * d_out: capacity n samples; *h_out_len = samples written. */
#define RT_STREAM_MEASURE    0x01u
#define RT_STREAM_TRIM_START 0x02u
#define RT_STREAM_TRIM_END   0x04u
#define RT_STREAM_FADE_IN    0x08u
#define RT_STREAM_FADE_OUT   0x10u
RT_API int rt_stream_chunk(rt_ctx* ctx, const rt_post_params* p, const float* d_in, int64_t n, uint32_t flags, double* h_dc_gain,
                           float* d_out, int64_t* h_out_len);
/* rt_stream_chunk for the chunks of several listeners at once: one upload, one launch (a workgroup per item), one download.
 *   h_in_ptr / h_out_ptr [n_items] device pointers, h_n / h_flags [n_items], h_dc_gain [n_items][2] in/out, h_out_len [n_items] out.
 * Every item gets exactly the samples, length, dc and gain that rt_stream_chunk gives it alone (the two kernels share one body).  An
 * item with n == 0 writes nothing and keeps its state (h_out_len 0). */
RT_API int rt_stream_chunks(rt_ctx* ctx, const rt_post_params* p, int32_t n_items, const float* const* h_in_ptr, const int64_t* h_n,
                            const uint32_t* h_flags, double* h_dc_gain, float* const* h_out_ptr, int64_t* h_out_len);

/* ------------------------------------------------------------------ model
 * Stands behind the third-party model object the reference drives
 * (providers/qwen.py:160-165 from_pretrained, :247-251 generate_custom_voice,
 * :253-258 generate_voice_clone): talker decode + residual-code predictor +
 * codec decoder, shape-parametrised (the real dimensions are UNVERIFIED offline).
 */
typedef struct rt_stack_dims {
    int32_t hidden, layers, heads, kv_heads, head_dim, inter;
    float rope_theta, rms_eps;
} rt_stack_dims;

/* Conditioning front-end (reference audio -> codes + speaker embedding): a causal conv encoder (filters x 2 per stage,
 * strides ratios[]), a transformer at twice the frame rate, a stride-2 conv and a split residual vector quantiser.
 * filters = 0: the model has no encoder (rt_voice_encode / rt_model_set_voice_pcm return RT_ERR_UNSUPPORTED). */
typedef struct rt_encoder_config {
    int32_t filters, n_ratios, ratios[8], kernel, res_kernel, last_kernel;
    rt_stack_dims tf;             /* hidden = encoder width                                  */
    int32_t window, vq_dim, spk_hidden;
    int32_t max_ref_frames;       /* longest reference clip, in codec frames                  */
} rt_encoder_config;

typedef struct rt_model_config {
    rt_stack_dims talker, predictor, codec_tf;
    int32_t codec_vocab, predictor_vocab, text_vocab, text_hidden, n_groups;
    int32_t codebook_size, num_quantizers, codec_sliding_window;
    int32_t n_upsampling;         /* ConvNeXt upsample stages            */
    int32_t upsampling_ratios[4];
    int32_t n_upsample_rates;     /* decoder blocks                      */
    int32_t upsample_rates[8];
    int32_t decoder_dim;
    int32_t codec_eos_id;
    int32_t max_batch;            /* sequences decoded together, 1..128  */
    int32_t max_positions;        /* KV rows per sequence (prompt + frames) */
    int32_t max_codec_frames;     /* frames per sequence one rt_code2wav call may decode */
    int32_t reserved[4];          /* [0]: max_voices, the entries of the voice bank (0 = 1, at most 8: rt_voice_select); [1..3]: 0 */
    rt_encoder_config enc;
} rt_model_config;

#define RT_DTYPE_BF16 0
#define RT_DTYPE_F32  1

typedef struct rt_sampling {
    int32_t do_sample;            /* 0: greedy (lowest index on ties)    */
    float   temperature;
    int32_t top_k;                /* 1..64 when sampling                 */
    float   top_p;
    float   repetition_penalty;   /* talker group 0 only                 */
} rt_sampling;

RT_API int rt_model_create(rt_ctx* ctx, const rt_model_config* cfg, rt_model** out_model);
RT_API int rt_model_destroy(rt_model* m);
/* Number of named tensors the model expects, and the name / shape of the i-th (INTEGRATION.md lists them). */
RT_API int rt_model_tensor_count(rt_model* m);
RT_API int rt_model_tensor_info(rt_model* m, int32_t index, char* name, size_t name_cap, int64_t* shape2, int32_t* kind);
/* Upload one tensor (matrices [N][K] row-major bf16; vectors bf16 or f32).  on_device != 0: data is an HBM pointer. */
RT_API int rt_model_set_tensor(rt_model* m, const char* name, const void* data, int32_t dtype, int64_t rows, int64_t cols,
                               int32_t on_device);
/* After the last tensor: verifies completeness, uploads RoPE tables (h_* are [max_positions][head_dim/2] float32,
 * one pair per stack: talker, predictor, codec_tf) and derives the projected predictor embedding tables. */
RT_API int rt_model_finalize(rt_model* m, const float* h_rope_cos[3], const float* h_rope_sin[3]);
RT_API int64_t rt_model_weight_bytes(rt_model* m);

/* Voice conditioning = the shared prompt prefix, computed ONCE per voice (the reference re-derives it on every
 * call by passing ref_audio=path each time, qwen.py:253-258).  Row recipe of the prefix, one entry per row:
 *   h_text_ids[r]   text token of the row, or -1 for tts_pad
 *   h_codec_ids[r*n_groups + g]  codec-side ids summed into the row (g = 0: talker table / control ids;
 *                   g >= 1: residual codebook g), -1 = none
 *   h_speaker_row   row that additionally receives h_speaker_embed[hidden] (float32), or -1
 */
RT_API int rt_model_set_voice(rt_model* m, int32_t n_rows, const int32_t* h_text_ids, const int32_t* h_codec_ids,
                              int32_t h_speaker_row, const float* h_speaker_embed);
/* The step BEFORE the path: the reference hands the model a reference-audio PATH on every call
 * (ref_audio=..., providers/qwen.py:253-258) and the model encodes it each time; here the clip is encoded once, on the GPU.
 *   h_pcm       mono float32 in [-1, 1] at the model's sample rate (host memory); n_samples is cut down to whole codec frames
 *   h_codes     out [n_frames][num_quantizers] (capacity max_frames rows), h_n_frames out
 *   h_speaker_embed  out [talker hidden] float32 (statistics-pooled speaker head), may be NULL */
RT_API int rt_voice_encode(rt_model* m, const float* h_pcm, int64_t n_samples, int32_t* h_codes, int32_t max_frames, int32_t* h_n_frames,
                           float* h_speaker_embed);
/* rt_voice_encode + rt_model_set_voice in one call: the recipe arrays describe the rows BEFORE the reference frames (role /
 * control / speaker / bos / reference-text rows, as for rt_model_set_voice); one row per encoded frame is appended, with text id
 * frame_text_id (tts_pad) and the frame's codes; the speaker row receives the encoder's speaker embedding.  Needs
 * num_quantizers == n_groups.  h_codes / h_n_frames (optional) return what was encoded. */
RT_API int rt_model_set_voice_pcm(rt_model* m, const float* h_pcm, int64_t n_samples, int32_t n_head_rows, const int32_t* h_text_ids,
                                  const int32_t* h_codec_ids, int32_t h_speaker_row, int32_t frame_text_id, int32_t max_ref_frames,
                                  int32_t* h_codes, int32_t* h_n_frames);
RT_API int32_t rt_voice_prefix_len(rt_model* m);
/* Prefix KV as one HBM blob [2][layers][kv_heads][prefix_len][head_dim] bf16, for an RCCL broadcast. */
RT_API int64_t rt_voice_blob_bytes(rt_model* m);
RT_API int rt_voice_export(rt_model* m, void* d_blob, int64_t bytes);
RT_API int rt_voice_import(rt_model* m, int32_t prefix_len, const void* d_blob, int64_t bytes);
/* The voice bank: a model holds rt_model_config.reserved[0] voices at once (max_voices; 0 means 1, at most 8 - a larger value fails
 * rt_model_create with RT_ERR_INVALID), voice v in talker cache slot max_batch + v with prefix tiles of its own.  Each extra voice
 * costs one cache slot plus two tile copies: 2 * layers * kv_heads * head_dim * 2 bytes * (max_positions + 32 * ceil(max_positions
 * / 32) [the tiles, head_dim 128 only]) - INTEGRATION.md works the figure out.  With max_voices 1 nothing is allocated that was
 * not before.
 *   rt_voice_capacity  max_voices.
 *   rt_voice_select    the entry that rt_model_set_voice, rt_model_set_voice_pcm, rt_voice_prefix_len, rt_voice_blob_bytes,
 *                      rt_voice_export and rt_voice_import act on, and the voice of every item of an rt_generate without item
 *                      voices.  Entry 0 until a caller selects another; host bookkeeping only, nothing is copied.
 *   rt_voice_clear     forgets an entry (its prefix length becomes 0: not set).
 *   rt_generate_item_voices  a voice per item for the NEXT rt_generate / rt_generate_begin, which consumes the array (the call after
 *                      it is a plain one again).  An item's codes are bit for bit the codes it gets alone with that voice selected.
 *                      Rows are dealt in 4-row blocks of one voice (rt_debug_voice_row_plan), so a run may decode on fewer busy rows
 *                      than a single-voice one.  Teacher forcing and the logit traces are refused with RT_ERR_UNSUPPORTED when the
 *                      items name more than one voice.
 * RT_ERR_INVALID: a voice outside 0 .. max_voices - 1, an item voice that is not set, n_items different from the generate call's.
 * RT_ERR_STATE: any of them while a generation is in flight. */
RT_API int32_t rt_voice_capacity(rt_model* m);
RT_API int rt_voice_select(rt_model* m, int32_t voice);
RT_API int rt_voice_clear(rt_model* m, int32_t voice);
RT_API int rt_generate_item_voices(rt_model* m, const int32_t* h_voice, int32_t n_items);
/* Of the last rt_generate: how many times a 4-row block whose rows had all come free was handed to another voice. */
RT_API int64_t rt_generate_revoiced_blocks(rt_model* m);

/* n_items may exceed the model's max_batch: the first max_batch items start on the decode rows, the others wait in a queue
 * (in array order - put the longest first) and take over a row as soon as the host has seen its item finish: the new item's
 * prompt suffix is prefilled into the row's KV slot between two frames (continuous batching).  An item's codes depend only
 * on (h_item_ids[i], seed), not on the row, the moment it ran or what it was batched with (bit for bit: tested at the 1.7B and
 * 0.6B shapes, first waves of fewer than 64, of 416 and of more than 1024 prompt rows - the prompt prefill runs in chunks of
 * <= 1024 rows on one kernel whose K association equals the <= 64-row kernel's; tests/test_model_shapes_gpu.py).  Teacher forcing and the logit traces need
 * n_items <= max_batch. */
typedef struct rt_generate_args {
    int32_t n_items;
    const int32_t* h_text_ids;      /* concatenated target-text token ids                          */
    const int32_t* h_text_offsets;  /* [n_items + 1]                                               */
    const int32_t* h_max_frames;    /* [n_items]                                                   */
    const int64_t* h_item_ids;      /* [n_items] RNG stream of each item (its global index)        */
    uint64_t seed;                  /* BaseTTS.seed (base_tts.py:45,142-149)                       */
    rt_sampling talker, predictor;
    int32_t ignore_eos;             /* synthetic weights never emit EOS: length = max_frames       */
    int32_t min_frames;
    int32_t tts_eos_id, tts_pad_id, codec_pad_id, codec_bos_id;
    const int32_t* h_forced_codes;  /* optional teacher forcing: item i frames at offset forced_offsets[i], [frames][n_groups] */
    const int32_t* h_forced_offsets;/* [n_items + 1], in frames                                    */
    const volatile int32_t* h_cancel_flag; /* polled between frames (CancellationToken, cancellation.py:19-65) */
    int32_t* h_codes;               /* out: item i at (sum_{j<i} max_frames[j]) * n_groups, [frames][n_groups] */
    int32_t* h_n_frames;            /* out: [n_items]                                              */
    float* d_trace_talker;          /* optional: [max_frames_max][n_items][codec_vocab] talker logits */
    float* d_trace_predictor;       /* optional: [max_frames_max][n_groups-1][n_items][predictor_vocab] */
    int32_t max_rows;               /* 0: decode on min(n_items, max_batch) rows; else on at most this many (a short queue is
                                       served faster by 32 busy rows than by 64 half-empty ones: a 64-row frame costs ~1.4x a
                                       32-row one)                                                                           */
} rt_generate_args;

RT_API int rt_generate(rt_model* m, const rt_generate_args* args);
/* The same generation in pieces (sub-segment streaming, SURVEY.md 8f-4: BaseTTS.stream, base_tts.py:1132-1190, hands audio over
 * per segment; here the first codec frames of a segment can be vocoded while the rest is still being decoded).
 *   rt_generate_begin   validates, prefills the prompts, builds the decode state; args->h_codes / h_n_frames may be NULL; every
 *                       input array is copied (only h_cancel_flag must stay valid until rt_generate_end).  A run that was
 *                       begun and never ended is dropped.
 *   rt_generate_step    runs up to n_frames more frames and returns once the host holds their codes; the next talker step is
 *                       already in flight on the stream.  *h_frames_run = frames run so far, *h_all_done = every item ended.
 *   rt_generate_peek    codes of `item` produced so far: frames [first_frame, first_frame + *h_n_frames) into h_codes
 *                       [max_frames][n_groups]; *h_finished = the item has ended.
 *   rt_generate_end     writes the results as rt_generate does (either pointer may be NULL) and releases the run; ending a run
 *                       that has not finished drops it (an error if results were asked for).
 * Between two steps other calls on the model are allowed (rt_code2wav of the frames already decoded); a voice change is not.
 * rt_generate == begin + one step of every frame + end: the codes are the same however the frames are cut into steps. */
RT_API int rt_generate_begin(rt_model* m, const rt_generate_args* args);
RT_API int rt_generate_step(rt_model* m, int32_t n_frames, int32_t* h_frames_run, int32_t* h_all_done);
RT_API int rt_generate_peek(rt_model* m, int32_t item, int32_t first_frame, int32_t max_frames, int32_t* h_codes, int32_t* h_n_frames,
                            int32_t* h_finished);
RT_API int rt_generate_end(rt_model* m, int32_t* h_codes, int32_t* h_n_frames);
/* Figures of the last rt_generate: decode frames launched, rows, frames kept over all items (row occupancy =
 * frames_kept / (frames_run * rows)) and the number of row hand-overs to queued items.  Any pointer may be NULL. */
RT_API int rt_generate_stats(rt_model* m, int64_t* frames_run, int64_t* rows, int64_t* frames_kept, int64_t* hand_overs);

/* An OPEN run: a generation whose item list grows while it decodes (a serving session: requests join a running batch).  Everything
 * that sizes a buffer is declared when the run is opened; the items come later, one rt_generate_submit each.  An item's codes are bit
 * for bit the codes it gets alone with its voice (rt_generate with one item), whatever else is on the rows and whenever it arrived.
 *   rows              decode rows of the run, 1 .. max_batch (they are all stepped every frame, busy or not)
 *   max_text_tokens   longest text of a later submit          max_frames   largest max_frames of a later submit
 *   horizon           frame-counter values the run may use (it sizes the code and end-of-sequence buffers: horizon * rows *
 *                     (n_groups + 1) * 4 bytes in HBM and as much on the host).  Frames are only counted while items decode.
 *   h_voices          [n_voices] the bank entries items may name (each set).  The run always takes the block-table form of a
 *                     multi-voice run (rt_generate_item_voices), and which attention launches a step takes is fixed by THIS list.
 *   seed, talker, predictor, ignore_eos, min_frames, the special ids, h_cancel_flag: of the run, as in rt_generate_args.
 *   n_items, h_text_ids, h_text_offsets, h_max_frames, h_item_ids, h_item_voices: an optional first list (n_items may be 0), each item
 *                     submitted in order as rt_generate_submit would.
 *   h_forced_codes, d_trace_talker, d_trace_predictor: must be NULL (RT_ERR_UNSUPPORTED).
 * rt_generate_submit appends one item and returns its index in *h_item (what rt_generate_peek takes).  The item gets a row at the
 * next hand-over look by the voice plan's rule (4-row blocks of one voice, submission order within a voice); until then it waits.
 * Refused, the run undisturbed: RT_ERR_INVALID - text longer or more frames than declared, a voice outside the declared list or not
 * set, a text id out of range; RT_ERR_LENGTH - prefix + text + frames exceed max_positions, or the remaining horizon cannot hold the
 * item ("horizon spent": let the run drain, end it and open another); RT_ERR_STATE - no run in flight, or a closed-list run.
 * rt_generate_cancel_item ends one item: its row is free at the next look, its frames so far stay readable, rt_generate_peek reports
 * it finished; nobody else's codes change.
 * rt_generate_step on an open run with nothing decoding and nothing waiting launches no frame and returns *h_all_done = 1; the run
 * stays open (RT_ERR_STATE, and the run is dropped, should it ever reach its horizon with items unfinished), and after a later submit the next step places the new items on the empty rows as a first wave is placed.
 * rt_generate_end closes the run (h_codes / h_n_frames as for rt_generate_begin: every submitted item must have ended);
 * rt_generate_stats then reports the whole run.  Only the host waits, and only for launched work: nothing spins on the device. */
typedef struct rt_generate_open_args {
    int32_t rows, max_text_tokens, max_frames, horizon;
    int32_t n_voices;
    const int32_t* h_voices;
    uint64_t seed;
    rt_sampling talker, predictor;
    int32_t ignore_eos, min_frames;
    int32_t tts_eos_id, tts_pad_id, codec_pad_id, codec_bos_id;
    const volatile int32_t* h_cancel_flag;
    int32_t n_items;
    const int32_t* h_text_ids;
    const int32_t* h_text_offsets;
    const int32_t* h_max_frames;
    const int64_t* h_item_ids;
    const int32_t* h_item_voices;
    const int32_t* h_forced_codes;
    float* d_trace_talker;
    float* d_trace_predictor;
} rt_generate_open_args;
RT_API int rt_generate_open(rt_model* m, const rt_generate_open_args* args);
RT_API int rt_generate_submit(rt_model* m, const int32_t* h_text_ids, int32_t n_text, int32_t max_frames, int64_t item_id, int32_t voice,
                              int32_t* h_item);
RT_API int rt_generate_cancel_item(rt_model* m, int32_t item);
/* Frames between two looks at the rows (hand-over cadence): of the run in flight, else what the next open run will take.  The bounds
 * of rt_generate_open / rt_generate_submit count 2 x this value of slack, and a caller that steps an open run steps by it. */
RT_API int32_t rt_generate_cadence(rt_model* m);

/* Codec decoder: h_codes [n_items][t_max][num_quantizers] (right-padded), h_n_frames [n_items];
 * d_wav [n_items][wav_stride] float32 in HBM, h_wav_len out.  rt_wav_length(frames) = samples produced. */
RT_API int64_t rt_wav_length(rt_model* m, int32_t n_frames);
RT_API int rt_code2wav(rt_model* m, int32_t n_items, int32_t t_max, const int32_t* h_codes, const int32_t* h_n_frames,
                       float* d_wav, int64_t wav_stride, int64_t* h_wav_len);

/* ------------------------------------------------------------------ speech-to-text for validation
 * Stands behind validation/stt/stt_validator.py:42-148 (_get_whisper_model / transcribe_audio: faster-whisper "tiny" on the CPU,
 * or transformers' Whisper - :85-107) and the temporary-WAV round trip of base_tts.py:821-830: a generated segment is
 * transcribed where it already lives, in HBM.  Whisper-shaped encoder-decoder, shape-parametrised:
 *   PCM (any rate) -> windowed-sinc resampler to `sample_rate` -> log-mel (n_fft-point DFT, hop, n_mels slaney filters, log10,
 *   (max - 8) floor, (x + 4) / 4; padded to chunk_seconds) -> conv k3 + conv k3 stride 2 (GELU) + positions -> enc_layers pre-LN
 *   layers -> dec_layers decoder layers (causal self-attention, cross-attention) -> tied LM head -> greedy ids after the forced
 *   prefix.  Tensor names and layouts: rt_stt_tensor_info; INTEGRATION.md lists them. */
typedef struct rt_stt rt_stt;
typedef struct rt_stt_config {
    int32_t d_model, heads, ffn, enc_layers, dec_layers;
    int32_t n_mels, n_ctx, n_text_ctx, vocab;          /* n_ctx: encoder positions (1500); n_text_ctx: decoder positions (448) */
    int32_t n_fft, hop, sample_rate, chunk_seconds;    /* 400, 160, 16000, 30: chunk_seconds * sample_rate / hop == 2 * n_ctx       */
    int32_t eos_id;
    int32_t n_prefix, prefix[8];                       /* forced decoder prefix (start-of-transcript, language, task, no-timestamps) */
    int32_t suppress_from;                             /* ids >= suppress_from are never produced, eos_id excepted (0: none)         */
    int32_t n_begin_suppress, begin_suppress[4];       /* ids not allowed as the FIRST generated token (space, end-of-sequence)      */
    int32_t max_new_tokens;
    int32_t reserved[4];
} rt_stt_config;
RT_API int rt_stt_create(rt_ctx* ctx, const rt_stt_config* cfg, rt_stt** out);
RT_API int rt_stt_destroy(rt_stt* s);
RT_API int rt_stt_tensor_count(rt_stt* s);
RT_API int rt_stt_tensor_info(rt_stt* s, int32_t index, char* name, size_t name_cap, int64_t* shape2, int32_t* kind);
RT_API int rt_stt_set_tensor(rt_stt* s, const char* name, const void* data, int32_t dtype, int64_t rows, int64_t cols, int32_t on_device);
RT_API int rt_stt_finalize(rt_stt* s);
/* Ids that are never produced, besides [suppress_from, vocab): the `suppress_tokens` list of a checkpoint's generation config.
 * Before rt_stt_finalize. */
RT_API int rt_stt_set_suppress(rt_stt* s, const int32_t* h_ids, int32_t n);
/* d_pcm: mono float32 in HBM at `sample_rate_in` (the TTS output as it stands).  h_tokens receives the ids generated after the
 * prefix, end-of-sequence excluded.  Audio longer than one chunk (chunk_seconds, 30 s) is NOT truncated: it is transcribed in
 * consecutive chunk_seconds windows (features, encoder, greedy decode behind the forced prefix per window, at most
 * cfg.max_new_tokens ids each) and the ids are concatenated, at most max_tokens in all - size h_tokens for
 * ceil(seconds / chunk_seconds) * cfg.max_new_tokens.  This is rt_stt_transcribe_batch with one clip: the clip's windows are the
 * rows of the same launches.  d_first_logits (optional, HBM, [vocab]): the logits behind the forced prefix of the FIRST window,
 * for tests. */
RT_API int rt_stt_transcribe(rt_stt* s, const float* d_pcm, int64_t n_samples, int32_t sample_rate_in, int32_t* h_tokens, int32_t max_tokens,
                             int32_t* h_n_tokens, float* d_first_logits);
/* n_clips clips in one call: d_pcm[i] holds n_samples[i] floats in HBM, all at sample_rate_in; h_tokens [n_clips][max_tokens_per_clip]
 * and h_n_tokens [n_clips] receive per clip exactly the ids it gets as the only clip of a call (rt_stt_transcribe) with max_tokens =
 * max_tokens_per_clip (size a row for ceil(seconds / chunk_seconds) * cfg.max_new_tokens).  Every clip is cut into chunk_seconds
 * windows as there, and the windows of all clips - 32 at a time - go through the front end, the encoder and the greedy decode
 * together: one launch per stage for the group, and one device-to-host read and one stream synchronisation per decode step
 * whatever the number of clips.  The handle holds ONE set of buffers for all rt_stt_* calls (78.7 MB per window measured at
 * Whisper-tiny dimensions): rt_stt_finalize reserves it for one window, the first call with more windows replaces it by a larger
 * one and it only grows; a handle that never batches holds one window's, and one whose allocation failed (out of memory) holds
 * none and allocates again at the next call.  n_clips == 0: nothing to do, RT_OK.
 * RT_ERR_INVALID: a null pointer for a clip with samples, a negative length, max_tokens_per_clip < 1.  A clip of zero samples is
 * one window of silence, as in rt_stt_transcribe. */
RT_API int rt_stt_transcribe_batch(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips, int32_t sample_rate_in,
                                   int32_t* h_tokens, int32_t max_tokens_per_clip, int32_t* h_n_tokens);
/* rt_stt_transcribe_batch decoded by beam search of width beam_size (1 .. 8; the rule: DESIGN.md section 5 - Whisper's published
 * BeamSearchDecoder with faster-whisper's defaults, patience 1 and length penalty 1, which is what the reference's
 * model.transcribe(path, language="en") runs with at width 5).  Per window: up to beam_size live hypotheses with cumulative
 * float32 log-probabilities (log-softmax over the whole vocabulary of the logits masked as for the greedy rule), beam_size + 1
 * candidates per hypothesis and step, a finished list of beam_size entries; the result is the entry with the largest
 * score / (ids + 1).  beam_size == 1 gives the ids of rt_stt_transcribe_batch.  floor(32 / beam_size) windows make a group, whose
 * decoder rows are windows x beams; a clip's ids and score do not depend on the other clips of the call.  Every window of a clip is
 * decoded and max_tokens cuts the joined ids.  h_scores (optional) [n_clips]: the clip's average log-probability per emitted token,
 * end-of-sequence counted: sum of its windows' cumulative log-probabilities / sum of (ids + 1).  The decoder side of the beam rows
 * (two self-attention caches, logits) is allocated by the first beam call and only grows.  RT_ERR_INVALID: the argument rules of
 * rt_stt_transcribe_batch, and a beam_size outside 1 .. 8. */
RT_API int rt_stt_transcribe_beam(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips, int32_t sample_rate_in,
                                  int32_t beam_size, int32_t* h_tokens, int32_t max_tokens, int32_t* h_n_tokens, float* h_scores);
/* Languages and silence ("language and no-speech").  For one window let z be the float32 logits over the whole
 * vocabulary behind start-of-transcript ALONE (one decoder row at position 0 over the window's encoder states, nothing suppressed):
 * the window's language is the configured id with the largest z (lowest id on ties, NaNs never), its probability the softmax of z
 * over the configured ids, and the no-speech probability softmax(z) over the whole vocabulary at the no-speech id.  A clip's
 * language is decided on its FIRST window and forced on every window of the clip.
 * rt_stt_set_languages: the ids position 1 of the forced prefix may take (1 .. 128 of them) and the no-speech id.  Before
 *   rt_stt_finalize, like rt_stt_set_suppress.  RT_ERR_INVALID: a configured prefix of fewer than two entries, prefix[1] not in the
 *   list, an id outside the vocabulary.  A handle without languages transcribes as before and refuses the calls below that need them.
 * rt_stt_detect_language: the first window of every clip through front end, encoder, probe pass and k_stt_probe, 32 windows at a
 *   time -> per clip the language id, its probability and the no-speech probability (the last two optional). */
RT_API int rt_stt_set_languages(rt_stt* s, const int32_t* h_lang_ids, int32_t n, int32_t no_speech_id);
RT_API int rt_stt_detect_language(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips, int32_t sample_rate_in,
                                  int32_t* h_lang, float* h_lang_prob, float* h_no_speech);
/* rt_stt_transcribe_beam with options and a fuller report.  All pointers are host memory.
 * opts: beam_size 1 .. 8 (1 gives the greedy ids); max_tokens caps every clip's joined ids; h_language [n_clips] or NULL - an entry
 *   >= 0 forces that configured language id on the clip, -1 detects it; NULL: the handle's prefix, and - unless h_win_no_speech is
 *   asked for - exactly the launches of rt_stt_transcribe_beam.  The probe pass (one more decoder pass of one row per window, and
 *   one workgroup per window) runs when a clip detects or h_win_no_speech is given; the windows' prefixes are then written on the
 *   device, with no host synchronisation before the prefix pass.  With every language given and no h_win_no_speech the prefixes
 *   are copied in and no launch is added to those of rt_stt_transcribe_beam.
 * out, per clip: h_tokens [n_clips][max_tokens], h_n_tokens, h_scores (optional) as rt_stt_transcribe_beam; h_language (optional)
 *   the id at position 1 of the clip's prefix; h_language_prob (optional) its probability where it was detected, 1 where it was given.
 *   Per window, in clip order, each optional, window_cap entries of room: h_win_clip the owning clip, h_win_n_ids the ids the window
 *   decoded (before max_tokens cuts the clip's joined ids), h_win_logprob its hypothesis' cumulative log-probability (avg_logprob =
 *   that / (ids + 1)), h_win_no_speech.  n_windows receives the number of windows.  The silence rule (a window is silent when
 *   no_speech > threshold and avg_logprob < threshold) is the host's: rho_tts_amd/validation.py.
 * RT_ERR_INVALID (nothing is launched, the handle stays usable): the argument rules of rt_stt_transcribe_beam; a language entry that
 *   is neither -1 nor a configured id; h_language or h_win_no_speech on a handle without rt_stt_set_languages; window_cap below the
 *   number of windows when a per-window array is given.  n_clips == 0: RT_OK, n_windows = 0. */
typedef struct rt_stt_decode_opts {
    const int32_t* h_language;
    int32_t beam_size, max_tokens;
    int32_t reserved[4];
} rt_stt_decode_opts;
typedef struct rt_stt_decode_out {
    int32_t* h_tokens;
    int32_t* h_n_tokens;
    float* h_scores;
    int32_t* h_language;
    float* h_language_prob;
    int32_t* h_win_clip;
    int32_t* h_win_n_ids;
    float* h_win_logprob;
    float* h_win_no_speech;
    int32_t window_cap, n_windows;
    int32_t reserved[4];
} rt_stt_decode_out;
RT_API int rt_stt_transcribe_ex(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips, int32_t sample_rate_in,
                                const rt_stt_decode_opts* opts, rt_stt_decode_out* out);
/* Clips longer than one window by timestamps and seek ("timestamps and seek"), as the reference's transcribers
 * walk them: every window is decoded WITH timestamp tokens under the step rule (transformers' WhisperTimeStampLogitsProcessor), and
 * the seek rule (_retrieve_segment) closes segments at timestamp pairs, discards an unfinished tail and starts the clip's next
 * window at the last closed pair's timestamp, so a word that straddles a boundary is decoded again whole.  Conditioning on
 * previous text and an initial prompt: rt_stt_set_prompt below (off by default).  Temperature fallback: rt_stt_set_fallback below.  A round holds one window per unfinished clip; rounds run in groups of
 * floor(32 / beam_size) windows as rt_stt_transcribe_beam.  A clip's result is what it gets as the only clip of a call.
 * rt_stt_set_timestamps: timestamp ids [timestamp_begin, timestamp_begin + n_timestamps), n_timestamps = chunk_seconds / 0.02 + 1;
 *   timestamp_begin - 1 is <|notimestamps|>.  Before rt_stt_finalize.  RT_ERR_INVALID: the vocabulary does not hold the ids, the
 *   handle's prefix does not end in timestamp_begin - 1, or end-of-sequence is not below it.  In timestamp mode the prefix is the
 *   handle's without that last entry and the timestamp ids leave the suppress mask - for rt_stt_transcribe_seek only; every other
 *   entry point is what it is without this call.
 * opts: beam_size, max_tokens (caps every clip's joined TEXT ids) and h_language as rt_stt_decode_opts; max_initial_timestamp_index
 *   (-1: no limit): the largest timestamp index a window's first token may take; no_speech_threshold (NaN: the silence rule is off)
 *   and logprob_threshold (NaN: the no-speech test alone): a window with no_speech > threshold and avg_logprob < threshold
 *   contributes no segment and is consumed whole.
 * out, per clip: h_tokens [n_clips][max_tokens] the text ids of the clip's segments joined (timestamps and end-of-sequence stripped,
 *   discarded tails not included), h_n_tokens, h_scores (optional; sum of the kept windows' cumulative log-probabilities / sum of
 *   their tokens + 1), h_language, h_language_prob (optional) as rt_stt_decode_out.  max_clip_tokens receives the largest uncut
 *   number of text ids of a clip.  Per segment, in clip order, each optional, segment_cap entries of room: the owning clip, start
 *   and end in seconds of the clip and in ticks (one tick = floor(0.02 sample_rate_in) input samples), the number of text ids.  Per
 *   window, in clip order, each optional, window_cap entries: the owning clip, the start offset in input samples, the ids decoded
 *   (timestamps counted), the cumulative log-probability, the no-speech probability (NaN when no probe ran), the advance in ticks.
 *   n_segments / n_windows receive the full counts.  Nothing is written past a cap: when one is too small the call returns
 *   RT_ERR_LENGTH with the counts a repeat needs.
 * RT_ERR_INVALID (nothing is launched, the handle stays usable): the argument rules of rt_stt_transcribe_ex; a handle without
 *   rt_stt_set_timestamps; a cap below 1; the silence rule, h_language or h_win_no_speech on a handle without rt_stt_set_languages. */
typedef struct rt_stt_seek_opts {
    const int32_t* h_language;
    int32_t beam_size, max_tokens;
    int32_t max_initial_timestamp_index;
    float no_speech_threshold, logprob_threshold;
    int32_t reserved[3];
} rt_stt_seek_opts;
typedef struct rt_stt_seek_out {
    int32_t* h_tokens;
    int32_t* h_n_tokens;
    float* h_scores;
    int32_t* h_language;
    float* h_language_prob;
    int32_t* h_seg_clip;
    float* h_seg_start;
    float* h_seg_end;
    int32_t* h_seg_start_tick;
    int32_t* h_seg_end_tick;
    int32_t* h_seg_n_ids;
    int32_t* h_win_clip;
    int64_t* h_win_offset;
    int32_t* h_win_n_ids;
    float* h_win_logprob;
    float* h_win_no_speech;
    int32_t* h_win_advance;
    int32_t segment_cap, window_cap, n_segments, n_windows, max_clip_tokens;
    int32_t reserved[3];
} rt_stt_seek_out;
RT_API int rt_stt_set_timestamps(rt_stt* s, int32_t timestamp_begin, int32_t n_timestamps);
RT_API int rt_stt_transcribe_seek(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips, int32_t sample_rate_in,
                                  const rt_stt_seek_opts* opts, rt_stt_seek_out* out);
/* Temperature fallback ("temperature fallback"; faster-whisper's generate_with_fallback, which the reference's
 * model.transcribe runs with temperatures 0, 0.2 .. 1.0, best_of 5, thresholds 2.4 and -1.0).  A policy applies to
 * rt_stt_transcribe_ex and rt_stt_transcribe_seek only.  Per window, over the temperatures in order: temperature 0 is the beam decode
 * at the call's beam_size; a temperature T > 0 decodes best_of independent sampled rows (Gumbel-max over the ids the step rule leaves,
 * scores on the untempered log-probabilities) and keeps the one with the largest score / (ids + 1).  An attempt needs another one when
 * ratio(text ids) > compression_ratio_threshold or score / (ids + 1) < logprob_threshold - unless no_speech_threshold and
 * logprob_threshold are both set, no_speech > no_speech_threshold and the average is below logprob_threshold: that window is silence
 * and the caller's silence rule deals with it.  The first attempt that needs no other is the window's result; when every temperature
 * failed it is the attempt with the largest average among those within the compression threshold (among all when none is), the
 * earliest on ties.  Later attempts decode over the encoder states the group still holds: no front-end or encoder launch is
 * repeated.  A group holds floor(32 / max(beam_size, best_of)) windows while a policy is set.  A window's draws are keyed by (seed,
 * window key, temperature index, sample index, step, id) - window key: the window's start in ticks (rt_stt_transcribe_seek) or its
 * index in its clip (rt_stt_transcribe_ex) - so a clip's result does not depend on the other clips of the call.
 * ratio: the compression ratio of one attempt's text ids (timestamps stripped), computed by the caller - the library links no zlib.
 *   It runs on the thread that called rt_stt_transcribe_ex / rt_stt_transcribe_seek, with the context's mutex held: it must NOT call
 *   back into the handle or its context.  A result that is NaN or <= 0 fails the call with RT_ERR_INVALID.  NULL: no compression test.
 * rt_stt_set_fallback: after rt_stt_finalize, between calls; NULL clears the policy.  With no policy set every entry point issues
 *   exactly the launches it issues without this feature and returns the same bits.  RT_ERR_INVALID (the policy is unchanged):
 *   n_temperatures outside 1 .. 8, best_of outside 1 .. 8, temperatures negative, not finite or not strictly ascending, a
 *   compression threshold without a callback, a no_speech_threshold on a handle without rt_stt_set_languages.
 * rt_stt_fallback_report: per window of the last rt_stt_transcribe_ex / rt_stt_transcribe_seek call under a policy, in the order of
 *   that call's per-window arrays: the attempts made, the temperature of the chosen attempt and its ratio (NaN without a callback).
 *   Each array optional; n_windows receives the count; RT_ERR_LENGTH (nothing past cap is written) when cap is below it. */
typedef float (*rt_stt_ratio_fn)(const int32_t* ids, int32_t n_ids, void* user);
typedef struct rt_stt_fallback {
    int32_t n_temperatures;            /* 1 .. 8 */
    float temperatures[8];             /* strictly ascending, >= 0; only the first may be 0 */
    int32_t best_of;                   /* 1 .. 8 */
    float compression_ratio_threshold; /* NaN: off */
    float logprob_threshold;           /* NaN: off */
    float no_speech_threshold;         /* NaN: off; needs rt_stt_set_languages */
    uint64_t seed;
    rt_stt_ratio_fn ratio;             /* NULL: the compression test is off */
    void* ratio_user;
    int32_t reserved[4];
} rt_stt_fallback;
RT_API int rt_stt_set_fallback(rt_stt* s, const rt_stt_fallback* f);
RT_API int rt_stt_fallback_report(rt_stt* s, int32_t cap, int32_t* h_attempts, float* h_temperature, float* h_ratio, int32_t* n_windows);
/* Conditioning on previous text and an initial prompt ("conditioning on previous text"; faster-whisper's
 * condition_on_previous_text, prompt_reset_on_temperature and initial_prompt, which the reference's model.transcribe runs with at True,
 * 0.5 and none).  A policy applies to rt_stt_transcribe_seek only: the fixed-cut calls decode a clip's windows side by side and have
 * no "previous".  A clip's history starts as the initial prompt; every window that is not silent adds the ids of its closed segments,
 * timestamps included (not a discarded tail, not a segment of no duration or without a text id).  A window's prompt is the history
 * behind the clip's reset mark, cut to its last n_text_ctx / 2 - 1 ids; a window with a prompt decodes behind
 * [sot_prev_id] + prompt + the timestamp-mode prefix, a window without one behind that prefix alone, in every attempt of a fallback
 * policy.  Prompt ids are not scored and are no part of the generated history the step rule reads.  The window's budget is
 * min(max_new_tokens, n_text_ctx - its prefix length).  After a window the mark moves to the end of the history when
 * condition_on_previous is 0 or the window's chosen attempt ran at a temperature above reset_on_temperature (0 without a fallback
 * policy).  A clip's result stays what it gets as the only clip of a call.
 * rt_stt_set_prompt: after rt_stt_finalize, between calls; NULL clears the policy; h_initial is copied.  With no policy set every
 *   entry point issues exactly the launches it issues without this feature and returns the same bits.  RT_ERR_INVALID (the policy is
 *   unchanged): a handle without rt_stt_set_timestamps; sot_prev_id outside the vocabulary or not above end-of-sequence; an initial id
 *   outside [0, vocab); a reset temperature that is negative or infinite; a policy that neither conditions nor carries an initial
 *   prompt; a text context without room for a prompt behind the forced prefix.
 * rt_stt_prompt_report: per window of the last rt_stt_transcribe_seek call under a policy, in the order of that call's per-window
 *   arrays: the length of the prompt the window used and whether the reset mark moved behind it.  Each array optional; n_windows
 *   receives the count; RT_ERR_LENGTH (nothing past cap is written) when cap is below it. */
typedef struct rt_stt_prompt {
    int32_t sot_prev_id;               /* <|startofprev|> */
    int32_t condition_on_previous;     /* 0 / 1 */
    float reset_on_temperature;        /* NaN: never reset */
    const int32_t* h_initial;          /* copied by the call; NULL / 0: none */
    int32_t n_initial;
    int32_t reserved[4];
} rt_stt_prompt;
RT_API int rt_stt_set_prompt(rt_stt* s, const rt_stt_prompt* p);
RT_API int rt_stt_prompt_report(rt_stt* s, int32_t cap, int32_t* h_prompt_len, int32_t* h_reset, int32_t* n_windows);
/* Token times of KNOWN text by dynamic time warping over cross-attention (Whisper's word-timestamp method; the definition and its
 * deviations: DESIGN.md section 5, "word times").  All h_ pointers are host memory.
 * rt_stt_set_alignment: n_heads (1 .. 32) pairs (decoder layer, head) in h_layer_head [n_heads][2] and the width of the median filter
 *   along time (odd, 1 .. 31; Whisper uses 7).  Before or after rt_stt_finalize; the buffers are allocated by the first rt_stt_align.
 *   RT_ERR_INVALID: a pair out of range, a pair given twice, an even width.
 * rt_stt_align: every entry of d_pcm / n_samples is ONE window of at most chunk_seconds (a later window of a long clip: d_pcm + offset);
 *   window w carries the text ids h_text_ids[h_text_offsets[w] .. h_text_offsets[w + 1]) - no timestamp ids, no end-of-sequence, at
 *   most n_text_ctx - n_prefix - 1 of them - and decodes them teacher-forced behind the handle's prefix (which ends in
 *   <|notimestamps|>), position 1 replaced by h_language[w] where h_language is given (a configured id; detection is not offered
 *   here).  Windows run in groups of up to 32; a window's results are bit for bit those it has as the only window of a call.
 *   A window with n ids has n + 1 alignment rows; row k predicts token k of ids + [end-of-sequence].  Outputs, each optional:
 *   h_token_frame [sum (n + 1)]: per row the frame (0.02 s each) at which the path enters it - a token's start is its own entry, its end
 *   the next one, the last entry of a window (the end-of-sequence row) the end of its last token; h_token_logprob [sum n]:
 *   log_softmax over the text ids [0, eos_id) of the row's logits at the token; h_n_frames [n_windows]: the frames F of the window,
 *   clamp(resampled length / hop / 2, 1, n_ctx).  A window WITHOUT ids has no entries in the first two (sums run over the others).
 *   RT_ERR_LENGTH: a window longer than chunk_seconds, too many ids.  RT_ERR_INVALID: an id outside [0, vocab) or not a text id
 *   (>= eos_id: a special or timestamp id has no log-probability over the text ids), a handle without rt_stt_set_alignment, a
 *   language that is not configured.  On any error nothing is launched and the handle stays usable.
 *   Memory: beside the group's buffers the first call allocates, and later calls grow, workspaces for the rows of the pass and the
 *   probabilities W as windows x heads x r_max x f_max floats, r_max and f_max the group's largest n + 1 and F: 380 MiB measured for 32
 *   windows of 30 s with 60 ids and 12 heads; the worst case - 32 windows of 30 s, 32 heads, 449 rows each - is 2.7 GB for W alone. */
typedef struct rt_stt_align_out {
    int32_t* h_token_frame;
    float* h_token_logprob;
    int32_t* h_n_frames;
    int32_t reserved[4];
} rt_stt_align_out;
RT_API int rt_stt_set_alignment(rt_stt* s, const int32_t* h_layer_head, int32_t n_heads, int32_t median_width);
RT_API int rt_stt_align(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_windows, int32_t sample_rate_in, const int32_t* h_text_ids,
                        const int32_t* h_text_offsets, const int32_t* h_language, rt_stt_align_out* out);
/* Stages on their own (tests): the log-mel features [2 n_ctx][n_mels] and the encoder states [n_ctx][d_model], float32 in HBM:
 * row 0 of the same front end and encoder with the clip as its only window.  Of a clip longer than chunk_seconds the first
 * chunk is kept, and the resampler's taps at its end see the samples behind it. */
RT_API int rt_stt_log_mel(rt_stt* s, const float* d_pcm, int64_t n_samples, int32_t sample_rate_in, float* d_mel);
RT_API int rt_stt_encode(rt_stt* s, const float* d_pcm, int64_t n_samples, int32_t sample_rate_in, float* d_states);

/* ------------------------------------------------------------------ drift-classifier features
 * Stands behind the front half of validation/classifier/trainer.py:23-96 (extract_features, _estimate_formants: librosa on a
 * temporary WAV): the per-sample work of the 30 hand-crafted dimensions, on the waveform where it lives.
 *   d_pcm: mono float32 in HBM at sample_rate_in; resampled to 16 kHz on the device (the speech-to-text front-end's resampler).
 *   h_mfcc_stats26: mean (13) then population standard deviation (13) over the frames of the 13 MFCCs (n_fft 2048, hop 512,
 *     zero-padded centre, periodic Hann, 128 slaney mel filters, power_to_db with top_db 80, orthonormal DCT-II).
 *   h_cmnd [n_frames][max_period - min_period + 1] float64 (optional, room for cmnd_cap_frames frames): the cumulative-mean-
 *     normalised difference function of probabilistic YIN per pitch frame (frame 2048, window 1024, hop 512, zero-padded
 *     centre) for the lags min_period .. max_period (rt_features_geometry).  rt_features_extract hands it to the caller; the
 *     trough statistics and the Viterbi pass that turn it into F0 are defined by the host functions observation_log_probs and
 *     viterbi_banded of rho_tts_amd/features.py, and run as HIP kernels with that definition in rt_features_extract_batch.
 *   h_lpc [lpc_order + 1] float64: Burg LPC of the pre-emphasised (0.97), symmetric-Hann-windowed 25-ms frame about the middle
 *     sample; the formants are the angles of its roots.
 * Frames: 1 + n16 / 512 for both (n16 = samples at 16 kHz).  Parity with librosa is UNPINNED (not installable offline).
 * rt_features_extract and rt_features_extract_batch are one path (one launch per stage for the clips of the call, one workspace
 * set per handle): the first is it with one clip and without pYIN's back half, so it needs no pitch model; it skips the
 * difference function when h_cmnd is NULL.  RT_ERR_INVALID: fewer than two samples, before or after resampling;
 * RT_ERR_LENGTH: cmnd_cap_frames below the clip's frame count. */
typedef struct rt_features rt_features;
RT_API int rt_features_create(rt_ctx* ctx, rt_features** out);
RT_API int rt_features_destroy(rt_features* f);
/* min / max period of probabilistic YIN for a search range [fmin, fmax] Hz at the rate the analysis ASSUMES (the reference
 * leaves librosa.pyin's default 22050 in place for 16-kHz audio, trainer.py:52): floor(sr / fmax), min(ceil(sr / fmin), 1023). */
RT_API int rt_features_geometry(int32_t pitch_sr, double fmin, double fmax, int32_t* min_period, int32_t* max_period);
RT_API int rt_features_extract(rt_features* f, const float* d_pcm, int64_t n_samples, int32_t sample_rate_in, int32_t min_period,
                               int32_t max_period, int32_t lpc_order, double* h_mfcc_stats26, int32_t* h_n_mfcc_frames, double* h_cmnd,
                               int32_t cmnd_cap_frames, int32_t* h_n_pitch_frames, double* h_lpc);

/* The pitch model of probabilistic YIN's back half, uploaded once per rt_features (rho_tts_amd/features.py pitch_model builds it
 * with the numpy expressions of the host definition, so the device compares and adds the host's own bits):
 *   h_thresholds, h_beta [n_thresholds]: the ascending trough thresholds and the prior mass of each;
 *   h_log_trans [2][2 half_width + 1][n_bins]: log(w_local[offset][to-bin] * p + tiny), p = stay (index 0) / switch (index 1)
 *     probability of the voicing, offset = from-bin - to-bin + half_width; h_log_init [2 n_bins] = log(p_init + tiny);
 *   log_tiny = log(tiny), the transition from every state outside the band;
 *   pitch_sr, fmin, bins_per_semitone: bin of a period = round(12 bins_per_semitone log2(pitch_sr / period / fmin)), clipped to
 *     0 .. n_bins; no_trough_prob: the mass the global minimum gets from the thresholds that are not above it.
 * n_bins <= 2000, n_thresholds <= 1024. */
RT_API int rt_features_set_pitch_model(rt_features* f, int32_t n_bins, int32_t half_width, int32_t n_thresholds, const double* h_thresholds,
                                       const double* h_beta, const double* h_log_trans, const double* h_log_init, double log_tiny,
                                       double pitch_sr, double fmin, int32_t bins_per_semitone, double no_trough_prob);
/* The whole feature extraction of n_clips waveforms in HBM (d_pcm[c]: n_samples[c] floats at sample_rate_in) in one call, with one
 * stream synchronisation and one set of device-to-host copies whatever n_clips is:
 *   h_mfcc_stats26 [n_clips][26], h_lpc [n_clips][lpc_order + 1]: per clip the bits rt_features_extract gives for it alone (the
 *     same path: no launch mixes clips, and a clip's workgroups do what they do when it is the only clip);
 *   h_states [n_clips][cap_frames] int32: the Viterbi state path of every clip (voiced pitch bin b = state b, unvoiced = n_bins + b;
 *     -1 behind the clip's last frame); h_n_pitch_frames [n_clips] = 1 + n16 / 512.
 * Every clip is checked on the host before anything is launched.  RT_ERR_INVALID: a clip below two samples, cap_frames below a
 * clip's frame count, no pitch model set, more than 2^20 frames or 65535 clips in one call. */
RT_API int rt_features_extract_batch(rt_features* f, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips,
                                     int32_t sample_rate_in, int32_t min_period, int32_t max_period, int32_t lpc_order,
                                     double* h_mfcc_stats26, double* h_lpc, int32_t* h_states, int32_t cap_frames, int32_t* h_n_pitch_frames);

/* ------------------------------------------------------------------ speed and pitch control
 * Stands behind BaseTTS._apply_speed_pitch (base_tts.py:618-650: torchaudio.functional.resample(audio, int(sr * speed), sr), then
 * torchaudio.functional.pitch_shift(audio, sr, steps)) for one mono clip in HBM: float32 in, float32 out, every intermediate in
 * float64.  The resampler (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) evaluates its taps per output sample instead of
 * materialising torchaudio's [new][orig + 2 width] filter bank; the pitch stage is STFT (512, hop 128, periodic Hann, reflect-padded
 * centre) -> phase vocoder at `rate`, phase accumulated in float64 -> inverse STFT over the window envelope -> resampler -> crop or
 * zero-pad to the length the stage was given.  Definition: torchaudio 2.x's algorithm in exact arithmetic (tests/speed_pitch_ref.py);
 * parity with the package is UNPINNED (not installable offline).
 *
 * EVERY integer decision is the host's: rt_speedpitch_plan carries them (rho_tts_amd/speedpitch.py plan() computes them with
 * torchaudio's own Python expressions) and the device decides no length.  rt_speedpitch_apply therefore only enqueues kernels on the
 * context's stream: no device-to-host copy, no synchronisation (a workspace that has to grow is reallocated first; workspaces never
 * shrink).  The plan is checked against what integer arithmetic can re-derive (coprime rates, the filter half-width, the resampled
 * lengths, the frame count) and the float-derived counts against `rate`; an inconsistent plan, or out_capacity below the result's
 * length, is RT_ERR_INVALID and nothing is written.
 *   speed stage (do_speed): g = gcd(int(sr * speed), sr), s_o = int(sr * speed) / g, s_n = sr / g, s_width = ceil(6 s_o / (0.99
 *     min(s_o, s_n))), s_len = ceil(s_n n_in / s_o); s_o == s_n (equal rates): the stage copies
 *   L: samples behind the speed stage (n_in without it) = samples written to d_out
 *   pitch stage (do_pitch, L >= 257): rate = 2^(-steps / 12), nf = 1 + L / 128 input frames, n_out = ceil(nf / rate) output frames,
 *     ls = round(L / rate) stretched samples, resampled by p_o : p_n = int(sr / rate) : sr reduced, p_width, p_len as above */
typedef struct rt_speedpitch rt_speedpitch;
typedef struct rt_speedpitch_plan {
    int32_t do_speed, do_pitch;
    int64_t s_o, s_n, s_width, s_len;
    int64_t L;
    int64_t nf, n_out, ls;
    int64_t p_o, p_n, p_width, p_len;
    double  rate;
} rt_speedpitch_plan;
RT_API int rt_speedpitch_create(rt_ctx* ctx, rt_speedpitch** out);
RT_API int rt_speedpitch_destroy(rt_speedpitch* sp);
/* d_in [n_in] and d_out [out_capacity >= plan->L] are distinct float32 buffers in HBM. */
RT_API int rt_speedpitch_apply(rt_speedpitch* sp, const float* d_in, int64_t n_in, const rt_speedpitch_plan* plan, float* d_out,
                               int64_t out_capacity);

/* ------------------------------------------------------------------ drift classifier: forest inference from exported tables
 * Stands behind validation/classifier/__init__.py:115-118 (`model.predict_proba(x)[0][1]` of the pickled scikit-learn model): a
 * CalibratedClassifierCV of random forests with one isotonic calibrator each - or a bare forest - as plain arrays, which
 * rho_tts_amd/forest.py documents, exports (export_sklearn), validates and DEFINES the arithmetic of (predict_host).  All indices count
 * through the whole model:
 *   h_forest_first [n_forests + 1]: forest c owns the trees h_forest_first[c] .. h_forest_first[c + 1] - 1 (1 .. 64 forests);
 *   h_tree_first [n_trees + 1]: tree t owns the nodes h_tree_first[t] .. h_tree_first[t + 1] - 1, its root first;
 *   h_node_feature [n_nodes]: the split feature, -1 for a leaf; h_node_value: the float64 threshold of a split node / the class-1
 *     fraction of a leaf; h_node_right: the right child of a split node, -1 for a leaf.  The left child of node k is k + 1;
 *   h_iso_first [n_calibrators + 1], h_iso_x, h_iso_y: the knots of calibrator c (= forest c's); n_calibrators = n_forests, or 0 for
 *     a single uncalibrated forest.
 * rt_forest_set_model re-checks on the host what keeps the kernels in bounds and every walk finite - contiguous non-empty ranges, every
 * child behind its parent and inside its own tree, split features below n_features, finite values, leaf fractions in [0, 1], strictly
 * increasing knots, at most 64 levels - and returns RT_ERR_INVALID before anything is uploaded when a condition fails (the model set
 * before stays).  It uploads once and may be called again to replace the model.
 * rt_forest_predict: h_x [n_rows][n_features] float64 -> h_prob [n_rows] float64, bit-equal to predict_host row by row whatever else
 * shares the call: features rounded to float32 and compared as doubles (`x <= threshold` goes left), a forest's leaf fractions summed
 * in tree order and divided by the tree count, clipped to the calibrator's knots and interpolated with np.interp's arithmetic, the
 * calibrated values summed in order and divided by their count.  One host-to-device copy, two launches, one device-to-host copy and
 * one stream synchronisation on the context's stream, whatever n_rows is; workspaces belong to the handle and only grow.
 * n_rows == 0: RT_OK, nothing touched.  RT_ERR_INVALID with no launch: no model set, n_rows < 0, a feature that is NaN, infinite or
 * beyond float32's range. */
typedef struct rt_forest rt_forest;
RT_API int rt_forest_create(rt_ctx* ctx, rt_forest** out);
RT_API int rt_forest_destroy(rt_forest* f);
RT_API int rt_forest_set_model(rt_forest* f, int32_t n_features, int32_t n_forests, const int32_t* h_forest_first, int32_t n_trees,
                               const int32_t* h_tree_first, int32_t n_nodes, const int32_t* h_node_feature, const int32_t* h_node_right,
                               const double* h_node_value, int32_t n_calibrators, const int32_t* h_iso_first, const double* h_iso_x,
                               const double* h_iso_y);
RT_API int rt_forest_predict(rt_forest* f, const double* h_x, int32_t n_rows, double* h_prob);

/* ------------------------------------------------------------------ drift classifier: fitting the forests
 * Stands behind the RandomForestClassifier fits of validation/classifier/trainer.py:217-230: every tree of every forest of a
 * cross-validated fit in ONE call, written in the table layout above (pre-order nodes, left child = k + 1, no calibrators - those
 * are host arithmetic on held-out predictions, rho_tts_amd/forest_train.py).  forest_train.py states the rules - counter-hash random
 * numbers, bootstrap multiplicities, the leaf conditions on distinct rows, the partial Fisher-Yates feature draw, the split score and
 * its tie rule, the midpoint threshold - and DEFINES the result (fit_host): the tables returned here equal it bit for bit, and a tree
 * does not depend on the other trees of the call.
 *   h_x [n][n_features] float64 (rounded to float32, compared as doubles), h_y [n] 0 / 1, h_member [n_forests][n]: row i takes part
 *   in forest c when h_member[c][i] != 0.  p->n_trees trees PER FOREST; max_features 0 = floor(sqrt(n_features)), at least 1.
 *   h_tree_first [n_forests * n_trees + 1], h_node_feature / h_node_right / h_node_value [node_cap]: caller-owned; *h_n_nodes
 *   receives the node count.  CAPACITY: a tree over m member rows has at most 2 * floor(m / min_samples_leaf) - 1 nodes (at least 1)
 *   and never more than 2^(max_depth + 1) - 1 - rt_forest_fit_capacity(p, m) is that bound - and node_cap must be at least the sum of
 *   the bounds of all trees of the call (RT_ERR_LENGTH otherwise, before any launch).
 * Refused with no launch - RT_ERR_INVALID: a null pointer, a feature that is NaN, infinite or beyond float32's range, a y outside
 * {0, 1}, a forest without members, n_trees < 1, min_samples_leaf < 1, min_samples_split < 2, max_features outside 0 .. n_features,
 * a class weight that is not positive and finite, more than 64 forests; RT_ERR_LENGTH: n > 16384, n_features > 1024, max_depth > 64,
 * node_cap below the bound.  One host-to-device copy, two launches (the per-feature rank table; one workgroup per tree), one
 * device-to-host copy and one stream synchronisation on the context's stream, whatever the sizes; the workspaces are the context's
 * and only grow.  No floating-point atomics, no grid-wide barrier; every device loop is bounded by the capacity or the depth bound. */
typedef struct rt_forest_fit_params {
    int32_t n_trees;               /* per forest */
    int32_t max_depth;
    int32_t min_samples_leaf;      /* distinct rows */
    int32_t min_samples_split;     /* distinct rows */
    int32_t max_features;          /* 0: floor(sqrt(n_features)), at least 1 */
    int32_t bootstrap;             /* 0: every member row once */
    double w0, w1;                 /* class weights */
    uint64_t seed;
} rt_forest_fit_params;
RT_API int64_t rt_forest_fit_capacity(const rt_forest_fit_params* p, int32_t n_members);
RT_API int rt_forest_fit(rt_ctx* ctx, const double* h_x, int32_t n, int32_t n_features, const uint8_t* h_y, const uint8_t* h_member,
                         int32_t n_forests, const rt_forest_fit_params* p, int32_t node_cap, int32_t* h_tree_first, int32_t* h_node_feature,
                         int32_t* h_node_right, double* h_node_value, int32_t* h_n_nodes);

/* ------------------------------------------------------------------ speaker embedding: the GE2E encoder
 * Stands behind resemblyzer's VoiceEncoder.embed_utterance(preprocess_wav(...)) as the reference calls it for the first 256 of the
 * drift classifier's 286 dimensions (validation/classifier/trainer.py:23-68) and for _compute_speaker_similarity
 * (base_tts.py:325-346), on the waveform where it lives.  The definition is resemblyzer 0.1.x restated; parity with resemblyzer is
 * UNPINNED (neither it, webrtcvad, librosa nor pretrained weights are available offline).  Stages, in order:
 *   resample to 16 kHz (the resampler of the speech-to-text and feature front ends);
 *   normalize_volume(-30 dBFS, increase_only): rms over the clip in float64; below -30 dBFS the clip is multiplied by
 *     10^((-30 - 20 log10 rms) / 20).  DEVIATION: rms == 0 leaves the clip unchanged (resemblyzer yields NaN);
 *   trim_long_silences, ONLY for a clip with voice flags: one 0 / 1 flag per 480-sample window of the 16-kHz clip, which resemblyzer
 *     takes from webrtcvad (mode 3) and this library from the caller - it restates no VAD.  The clip is cut to a multiple of 480,
 *     the flags are averaged over 8 windows (3 zeros in front, 4 behind), rounded half to even, dilated by seven ones, and the
 *     windows whose mask is 1 are kept.  DEVIATION (the default): without flags nothing is cut.  A mask that keeps nothing gives one
 *     partial of zeros;
 *   partial utterances (rate 1.3, min_coverage 0.75): n_frames = ceil((n + 1) / 160), partial i = mel frames [77 i, 77 i + 160) for
 *     77 i < max(1, n_frames - 160 + 77 + 1); the last is dropped when it covers less than 0.75 of its 25600 samples and is not the
 *     only one; the clip is zero-padded to the last partial's end;
 *   mel: n_fft 400, hop 160, zero-padded centre, periodic Hann, float64 DFT, power spectrum, 40 slaney filters to 8 kHz, no log;
 *   torch.nn.LSTM(40, 256, num_layers = 3) from a zero state (gates i, f, g, o; two biases), per partial
 *     e = relu(W h_T + b), e / |e|; per clip the mean of its partial embeddings, divided by its norm (zero norm: zeros, not NaN).
 * rt_spk_set_tensor takes float32 host arrays under torch's names - lstm.weight_ih_l{0,1,2} [1024][40 | 256], lstm.weight_hh_l*
 * [1024][256], lstm.bias_ih_l*, lstm.bias_hh_l* [1024][1], linear.weight [256][256], linear.bias [256][1] - and the two front-end
 * tables mel.filters [201][40] and mel.window [400][1]; a wrong name or shape or a value that is not finite is RT_ERR_INVALID.
 * rt_spk_finalize packs and uploads them (RT_ERR_STATE when one is missing); calls before it are RT_ERR_STATE.
 * rt_spk_embed_batch: n_clips waveforms in HBM (d_pcm[c]: n_samples[c] floats at sample_rate_in) -> h_embed [n_clips][256] float32 and
 * h_n_partials [n_clips], with one launch per stage (the recurrent stage: one per layer, over tiles of 16 partials from whichever
 * clips), one stream synchronisation and one set of copies whatever n_clips is.  A clip's bits are the same alone, in any batch
 * and at any place in it.  h_voice_flags may be NULL (no clip is trimmed) and so may any h_voice_flags[c]; n_voice_flags[c] must
 * then be the clip's window count n16 / 480.  Every clip is checked on the host before anything is launched.  RT_ERR_INVALID: an
 * empty clip, a flag count that differs from n16 / 480, more than 65535 clips or 4096 partials in one call. */
typedef struct rt_spk rt_spk;
RT_API int rt_spk_create(rt_ctx* ctx, rt_spk** out);
RT_API int rt_spk_destroy(rt_spk* s);
RT_API int rt_spk_set_tensor(rt_spk* s, const char* name, const float* h_data, int64_t rows, int64_t cols);
RT_API int rt_spk_finalize(rt_spk* s);
RT_API int rt_spk_embed_batch(rt_spk* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips, int32_t sample_rate_in,
                              const uint8_t* const* h_voice_flags, const int32_t* n_voice_flags, float* h_embed, int32_t* h_n_partials);

/* Measurement and test entry points (rt_profile_*, rt_debug_*, rt_bench_*) are declared in rho_tts_amd_debug.h: a host binding of
 * the generation path needs none of them. */

#ifdef __cplusplus
}
#endif
#endif /* RHO_TTS_AMD_H */
