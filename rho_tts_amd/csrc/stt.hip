// On-GPU speech-to-text for the validation loop: a Whisper-shaped encoder-decoder behind the C ABI, so that a
// generated segment is transcribed where it already lives - in HBM - instead of going through a temporary WAV file and a CPU
// model.  Stands behind validation/stt/stt_validator.py:42-148 (model load, transcribe_audio; the reference's own fallback is
// transformers' Whisper, :85-107) and the temp-WAV round trip of base_tts.py:821-830.
//
//   PCM at the TTS rate -> windowed-sinc resampler (16 kHz; resample.h) -> log-mel front-end (400-point DFT per frame in float64, 80 slaney mel
//   filters, log10, (max - 8) floor, (x + 4) / 4: WhisperFeatureExtractor) -> 2 convs (GELU) + sinusoidal positions -> pre-LN
//   encoder (bidirectional attention over 1500 positions) -> decoder (causal self-attention + cross-attention, KV caches) ->
//   tied LM head -> greedy token ids after the forced prefix.
//
// Every GEMM is the tiled MFMA kernel of gemm.hip with float32 activations fed as hi + lo bf16 planes (weights bf16), K/V caches
// keep hi + lo planes and attention / LayerNorm run in float32: the token ids must equal the float32 oracle's (greedy argmax over
// 51865 logits), which plain bf16 activations would not guarantee.  The model is tiny (39 M parameters); nothing here is on the
// hot path of generation - it runs once per validated segment - so the kernels are the simple forms.
//
// There is one path.  Every entry point cuts its clips into chunk_seconds windows (stt_cut) and sends them, STT_GROUP at a time, as
// the rows of every launch: one front-end launch per stage for the group, one cache slot per window, one pick per row and step
// (k_stt_pick).  rt_stt_transcribe, rt_stt_log_mel and rt_stt_encode are that path with one clip; rt_stt_transcribe_batch is it with
// a whole validation chunk.  No launch mixes rows, so a clip's values among N rows are bit for bit those it has as the only row.
// The handle holds one buffer set (SttGroup: an encoder side and a greedy decoder side), reserved for one window at
// rt_stt_finalize and grown by the first call that needs more windows.
//
// rt_stt_transcribe_beam decodes the same windows by beam search (the reference's transcriber runs faster-whisper's default, width
// 5): decoder rows are windows x beams - a decoder side of its own (SttBeam) over the group's encoder side - k_stt_beam_select keeps
// the hypotheses on the device and k_stt_beam_reorder hands a row the self-attention cache of the row it continues; the call also
// returns each clip's average log-probability per emitted token.
//
// rt_stt_transcribe_ex is that beam path with a prefix per window: a probe pass (start-of-transcript alone, one row per window, the
// same stt_decode_rows) in front of the prefix pass, k_stt_probe reads a window's language and no-speech probability off its logits
// and k_stt_lang_prefix writes position 1 of every window's prefix on the device.  The three older entry points pass the handle's
// prefix and no probe: their launches are what they were.
//
// rt_stt_transcribe_seek walks a clip longer than a window as the reference's transcriber does ("timestamps and
// seek"): windows are decoded with timestamp tokens - k_stt_beam_select<true> applies the step rule in the passes the step already
// makes, from three facts per row kept in the beam book - and the host applies the seek rule to what a group decoded
// (stt_seek_rule): a round holds one window per unfinished clip at the clip's current offset, and the number of rounds is bounded
// before the first launch.  Off unless rt_stt_set_timestamps was called; no other entry point changes.
//
// rt_stt_set_fallback gives rt_stt_transcribe_ex and rt_stt_transcribe_seek the temperature fallback of the reference's transcriber
// ("temperature fallback"): after a group is decoded the host evaluates the rule per window (stt_fallback_group;
// the compression ratio is the caller's callback), and the windows that need another attempt are decoded again by sampling -
// best_of rows per window, k_stt_sample_select: Gumbel-max over the ids the step rules leave - over the encoder states the group
// still holds.  Off unless a policy is set; no other entry point changes.
// The decoding step rule - the ids a row may take, its normaliser, "timestamps win", the next history state - is stated once
// (stt_step_ids, stt_step_kind, stt_row_norm, stt_ts_next) and called by both select kernels; the two group decoders share the book's
// reset, the tail of a step and the book's fetch (stt_book_reset, stt_step_live, stt_book_fetch).
//
// rt_stt_set_prompt gives rt_stt_transcribe_seek the reference's conditioning on previous text and an initial prompt (DESIGN.md section
// 5, "conditioning on previous text"): the host keeps a history and a reset mark per clip, and a window with a prompt decodes behind
// <|startofprev|> + prompt + prefix.  The windows of a group then have prefixes of different lengths: one ragged prefix pass over
// sum(P_w) rows under row tables (stt_prompt_tables, stt_decode_tab), per-window positions and budgets at every step (k_stt_retire),
// and a gather between beam steps that moves generated positions only (k_stt_beam_reorder_range).  Off unless a policy is set; no
// other entry point changes.
//
// rt_stt_align gives the times of KNOWN text ("word times"): one teacher-forced pass over a group's windows with
// their text ids behind the prefix, during which stt_layer's capture argument has the kernels of stt_align.hip write the cross-attention
// probabilities of the alignment heads (rt_stt_set_alignment) out beside the unchanged attention launch; normalisation, median filter and
// head mean, and the monotone token-to-frame path by dynamic time warping follow on the device.  Nothing of it exists until the first
// call; the capture argument is null everywhere else, and no other entry point changes.
//
// The three beam entry points run their groups through one driver (stt_run_group) under one plan (SttPlan: the clips' language
// requests, whether the probe runs, the timestamp rule); what each keeps for itself is how it forms its groups and what it makes of
// the hypotheses - fixed cuts and joined ids (stt_transcribe_beam), rounds, offsets and the seek rule (stt_transcribe_seek).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

#include "kernels.h"
#include "knobs.h"
#include "resample.h"

namespace {

enum SttKind { S_GEMM = 0, S_VEC = 1, S_TABLE = 2 };
struct SttSlot {
    std::string name;
    int kind = 0;
    int64_t rows = 0, cols = 0;
    bool set = false;
    PackedW pw;
    float* vec = nullptr;
    bf16_t* tbl = nullptr;
    void* raw = nullptr;
    void* raw2 = nullptr;    // TABLE slots that are also multiplied (tied LM head): the packed copy
};

__global__ void k_stt_bf16_to_f32(const bf16_t* __restrict__ x, int64_t n, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = bf16_to_f32(x[i]);
}

// One window of a group, as the front-end kernels see it (a small device table, one entry per window)
struct SttWin {
    const float* pcm_in;    // the window's samples at the input rate
    const float* pcm16;     // ... at cfg.sample_rate: its row of the resampler's output, or pcm_in itself when the rates agree
    int64_t n_in, n16;      // samples at the input rate (the taps see all of them) / at cfg.sample_rate (at most one chunk)
    int32_t n_comp, pad;    // log-mel frames that can see audio; the rest hold the constant of silence
};
// the resampler over a group: blockIdx.y = window, its output row at y + window * y_stride
__global__ void k_resample_group(const SttWin* __restrict__ wins, float* __restrict__ y, int64_t y_stride, int L, int M, int taps, int half,
                                 const float* __restrict__ h) {
    const SttWin w = wins[blockIdx.y];
    float* yw = y + (int64_t)blockIdx.y * y_stride;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < w.n16; n += (int64_t)gridDim.x * blockDim.x)
        yw[n] = resample_at(w.pcm_in, w.n_in, n, L, M, taps, half, h);
}

// One frame per workgroup: the frame's 400 samples of the (zero-padded to 30 s, reflect-padded by n_fft / 2 at both ends) signal
// times the periodic Hann window, a direct DFT in float64 (bin k on thread k, twiddles from a 400-entry table: index k n mod 400),
// power spectrum, mel filters, log10(max(., 1e-10)).  logspec is [frames][n_mels]; gmax receives the maximum (ordered-int atomic).
__device__ __forceinline__ void logmel_frame(double* sh /* xw[n_fft] | c[n_fft] | s[n_fft] | power[n_bins] */, const float* __restrict__ pcm, int64_t n_valid,
                                             int64_t n_padded, int f, int n_fft, int hop, int n_bins, int n_mels, const double* __restrict__ twc,
                                             const double* __restrict__ tws, const float* __restrict__ window, const float* __restrict__ melT,
                                             float* __restrict__ logspec, int* __restrict__ gmax) {
    double* xw = sh;
    double* tc = sh + n_fft;
    double* ts = tc + n_fft;
    double* pw = ts + n_fft;
    const int tid = threadIdx.x;
    const int64_t start = (int64_t)f * hop - n_fft / 2;
    for (int n = tid; n < n_fft; n += blockDim.x) {
        int64_t t = start + n;
        if (t < 0) t = -t;                                // reflect (no edge repeat) about sample 0 ...
        if (t >= n_padded) t = 2 * (n_padded - 1) - t;    // ... and about the last sample of the padded signal
        const float v = (t >= 0 && t < n_valid) ? pcm[t] : 0.f;
        xw[n] = (double)(v * window[n]);                  // float32 product, as torch.stft applies its float32 window
        tc[n] = twc[n];
        ts[n] = tws[n];
    }
    __syncthreads();
    for (int k = tid; k < n_bins; k += blockDim.x) {
        double re = 0.0, im = 0.0;
        int idx = 0;
        for (int n = 0; n < n_fft; ++n) {
            re += xw[n] * tc[idx];
            im -= xw[n] * ts[idx];
            idx += k;
            if (idx >= n_fft) idx -= n_fft;
        }
        pw[k] = (double)((float)re * (float)re + (float)im * (float)im);   // |X|^2 from the float32 spectrum
    }
    __syncthreads();
    float best = -INFINITY;
    for (int m = tid; m < n_mels; m += blockDim.x) {
        double acc = 0.0;
        for (int k = 0; k < n_bins; ++k) acc += (double)melT[(int64_t)k * n_mels + m] * pw[k];
        const float v = log10f(fmaxf((float)acc, 1e-10f));
        logspec[(int64_t)f * n_mels + m] = v;
        best = fmaxf(best, v);
    }
    best = wave_max_f32(best);
    if ((tid & 63) == 0 && best > -INFINITY) atomicMax(gmax, f32_ordered(best));
}
// the frames of a group: blockIdx = (frame, window); window b's features at logspec + b * spec_stride, its maximum in gmax[b]
__global__ __launch_bounds__(256) void k_logmel_frames_group(const SttWin* __restrict__ wins, int64_t n_padded, int n_fft, int hop, int n_bins, int n_mels,
                                                             const double* __restrict__ twc, const double* __restrict__ tws,
                                                             const float* __restrict__ window, const float* __restrict__ melT /*[n_bins][n_mels]*/,
                                                             float* __restrict__ logspec, int64_t spec_stride, int* __restrict__ gmax) {
    extern __shared__ double sh[];
    const SttWin w = wins[blockIdx.y];
    if ((int)blockIdx.x >= w.n_comp) return;              // (uniform over the workgroup)
    logmel_frame(sh, w.pcm16, w.n16, n_padded, blockIdx.x, n_fft, hop, n_bins, n_mels, twc, tws, window, melT, logspec + (int64_t)blockIdx.y * spec_stride,
                 gmax + blockIdx.y);
}
// logspec[f][m] <- (max(v, gmax - 8) + 4) / 4; frames >= n_frames_audio hold the value of silence, log10(1e-10) = -10
__device__ __forceinline__ void logmel_finish(float* __restrict__ logspec, int64_t n_total, int64_t n_computed, const int* __restrict__ gmax) {
    const float mx = fmaxf(ordered_f32(*gmax), n_computed < n_total ? -10.f : -INFINITY);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_total; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = i < n_computed ? logspec[i] : -10.f;
        logspec[i] = (fmaxf(v, mx - 8.0f) + 4.0f) / 4.0f;
    }
}
__global__ void k_logmel_finish_group(const SttWin* __restrict__ wins, float* __restrict__ logspec, int64_t n_total, int n_mels, const int* __restrict__ gmax) {
    logmel_finish(logspec + (int64_t)blockIdx.y * n_total, n_total, (int64_t)wins[blockIdx.y].n_comp * n_mels, gmax + blockIdx.y);
}

// LayerNorm with bias over the last dimension, float32 in and out, one workgroup per row (two-pass: mean, then variance); input
// rows lie ldx elements apart (the last prefix row of every window of a group), output rows are dense
__global__ __launch_bounds__(256) void k_layernorm(const float* __restrict__ x, int64_t ldx, int D, const float* __restrict__ w, const float* __restrict__ b,
                                                   float eps, float* __restrict__ out) {
    __shared__ float sh[4];
    const float* r = x + (int64_t)blockIdx.x * ldx;
    float s = 0.f;
    for (int i = threadIdx.x; i < D; i += 256) s += r[i];
    s = wave_sum_f32(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    const float mean = (sh[0] + sh[1] + sh[2] + sh[3]) / (float)D;
    __syncthreads();
    float q = 0.f;
    for (int i = threadIdx.x; i < D; i += 256) { const float d = r[i] - mean; q += d * d; }
    q = wave_sum_f32(q);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = q;
    __syncthreads();
    const float inv = rsqrtf((sh[0] + sh[1] + sh[2] + sh[3]) / (float)D + eps);
    float* o = out + (int64_t)blockIdx.x * D;
    for (int i = threadIdx.x; i < D; i += 256) o[i] = (r[i] - mean) * inv * w[i] + b[i];
}

// x[r][:] = token_embedding[tok[r]] (bf16) + position_embedding[pos0 + r % per] (f32): `per` consecutive rows per window
__global__ void k_stt_embed(const bf16_t* __restrict__ tok_emb, const float* __restrict__ pos_emb, const int32_t* __restrict__ tok, int pos0, int per, int D,
                            float* __restrict__ x) {
    const int r = blockIdx.x;
    const int64_t t = tok[r];
    const int64_t pos = pos0 + r % per;
    for (int i = threadIdx.x; i < D; i += blockDim.x) x[(int64_t)r * D + i] = bf16_to_f32(tok_emb[t * D + i]) + pos_emb[pos * D + i];
}

// A group's greedy step, one 1024-thread workgroup per window: the row's next input token is the largest logit among the tokens the
// mask allows (bit 0: never, bit 1: not as the first generated token), lowest index on ties, NaNs never.  The host reads the group's
// tokens once per step and keeps the books; a row that has ended rides along as a dead row: it keeps writing its own cache slot and
// its own logits, nothing a live row reads.
__global__ __launch_bounds__(1024) void k_stt_pick(const float* __restrict__ all_logits, int V, const uint8_t* __restrict__ mask, int first_step,
                                                   int32_t* __restrict__ next_tok) {
    __shared__ float sv[16];
    __shared__ int si[16];
    const float* logits = all_logits + (int64_t)blockIdx.x * V;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    const uint8_t bad = first_step ? 3 : 1;
    for (int i = threadIdx.x; i < V; i += 1024) {
        if (mask[i] & bad) continue;
        const float v = logits[i];
        if (v > best || (v == best && i < bi) || bi == 0x7fffffff) { if (!(v != v)) { best = v; bi = i; } }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 16; ++w)
        if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
    next_tok[blockIdx.x] = bi == 0x7fffffff ? 0 : bi;
}

// What a window sounds like before anything is forced on it ("language and no-speech"), one 1024-thread
// workgroup per window over z, the logits behind start-of-transcript alone (no suppression mask): the configured language id with
// the largest z (lowest id on ties, NaNs never), its softmax over the configured ids, and softmax(z) over the whole vocabulary at
// the no-speech id.  NaNs take no part in either sum.  Every reduction has a fixed order - the <= 128 language terms one after the
// other on thread 0, the vocabulary per thread in index order, butterfly per wave, the 16 wave sums in wave order - so a window's
// three results do not depend on what it is batched with.  Row w of the logits starts at w * row_stride.
constexpr int STT_LANG_MAX = 128;                      // configured language ids (rt_stt_set_languages)
constexpr int STT_NO_LANG = 0x7fffffff;
__global__ __launch_bounds__(1024) void k_stt_probe(const float* __restrict__ all_logits, int64_t row_stride, int V, const int32_t* __restrict__ lang_ids, int n_lang,
                                                    int no_speech_id, int32_t* __restrict__ out_lang, float* __restrict__ out_lang_prob,
                                                    float* __restrict__ out_no_speech) {
    __shared__ float red[16];
    __shared__ float lz[STT_LANG_MAX];
    __shared__ int li[STT_LANG_MAX];
    const float* z = all_logits + (int64_t)blockIdx.x * row_stride;
    const int tid = threadIdx.x, wave = tid >> 6;
    if (tid < n_lang) { li[tid] = lang_ids[tid]; lz[tid] = z[li[tid]]; }
    float m = -INFINITY;
    for (int i = tid; i < V; i += 1024) { const float v = z[i]; if (v > m) m = v; }                  // (a NaN compares false)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((tid & 63) == 0) red[wave] = m;
    __syncthreads();
    m = red[0];
    for (int k = 1; k < 16; ++k) m = fmaxf(m, red[k]);
    __syncthreads();
    float sum = 0.f;
    for (int i = tid; i < V; i += 1024) { const float v = z[i]; if (v == v) sum += expf(v - m); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((tid & 63) == 0) red[wave] = sum;
    __syncthreads();
    if (tid != 0) return;
    sum = red[0];
    for (int k = 1; k < 16; ++k) sum += red[k];
    const float zn = z[no_speech_id];
    out_no_speech[blockIdx.x] = (m > -INFINITY && zn == zn) ? expf(zn - (m + logf(sum))) : 0.f;
    float best = -INFINITY;
    int bi = STT_NO_LANG;
    for (int k = 0; k < n_lang; ++k) {
        const float v = lz[k];
        if (v != v) continue;
        if (bi == STT_NO_LANG || v > best || (v == best && li[k] < bi)) { best = v; bi = li[k]; }
    }
    float ls = 0.f;
    for (int k = 0; k < n_lang; ++k)
        if (lz[k] == lz[k]) ls += expf(lz[k] - best);
    int low = li[0];                                       // no language has a number: the lowest configured id, probability 0
    for (int k = 1; k < n_lang; ++k) low = min(low, li[k]);
    out_lang[blockIdx.x] = bi == STT_NO_LANG ? low : bi;
    out_lang_prob[blockIdx.x] = (bi != STT_NO_LANG && best > -INFINITY) ? 1.0f / ls : 0.f;
}

// The forced prefix of every window of a group, written on the device behind k_stt_probe (no host round trip in between): the
// handle's prefix with position 1 replaced by the clip's language.  clip_lang[c] >= 0: the id the caller forced on clip c, or the id
// an earlier group of this call detected on its first window; -1: detect - then win_first[w] is the row, in this group, of the first
// window of w's clip, whose detected id every window of the clip takes (and clip_lang keeps it for the groups to come).
__global__ void k_stt_lang_prefix(int nW, int P, const int32_t* __restrict__ base_prefix, const int32_t* __restrict__ win_clip,
                                  const int32_t* __restrict__ win_first, int32_t* __restrict__ clip_lang, const int32_t* __restrict__ probe_lang,
                                  int32_t* __restrict__ prefix, int32_t* __restrict__ win_lang) {
    const int w = threadIdx.x;
    int lang = 0, clip = 0, first = -1;
    if (w < nW) {
        clip = win_clip[w];
        first = win_first[w];
        lang = clip_lang[clip];
        if (lang < 0) lang = first >= 0 ? probe_lang[first] : base_prefix[1];
    }
    __syncthreads();                                       // (every read of clip_lang lies before the writes)
    if (w >= nW) return;
    if (first == w) clip_lang[clip] = lang;
    win_lang[w] = lang;
    for (int i = 0; i < P; ++i) prefix[w * P + i] = i == 1 ? lang : base_prefix[i];
}

__global__ void k_stt_fill_i32(int32_t* p, int n, int v, int step) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = v + i * step;
}

// row i of a group's row tables: slot[i] = i / per (the window), pos[i] = i % per
__global__ void k_stt_fill_rows(int32_t* __restrict__ slot, int32_t* __restrict__ pos, int n, int per) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) { slot[i] = i / per; pos[i] = i % per; }
}
// dst[b][i] = src[i], b < reps: the encoder's positions laid under every window of a group
__global__ void k_stt_repeat(const float* __restrict__ src, int64_t n, int reps, float* __restrict__ dst) {
    const int64_t total = n * reps;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i % n];
}

// ---------------------------------------------------------------------------------------------- beam search (rt_stt_transcribe_beam)
// The decoding rule: per window up to B live beams with cumulative float32 log-probabilities and a finished
// list of at most B entries.  Decoder rows are windows x beams: row w B + j is beam j of window w.
constexpr int STT_BEAM_MAX = 8;
constexpr int STT_CAND = STT_BEAM_MAX + 1;              // candidates a beam contributes per step: B + 1 <= 9
constexpr int STT_NO_ID = 0x7fffffff;
constexpr int STT_SEL_U = 4;                            // logits a thread of k_stt_beam_select requests per round trip

// the order of one row's candidates: the larger log-probability first, the lower id on ties (NaNs never enter)
__device__ __forceinline__ bool cand_before(float v, int i, float ov, int oi) { return v > ov || (v == ov && i < oi); }

// The beam bookkeeping of a group, one int32 allocation of `R` rows (R >= windows x B): what k_stt_beam_select keeps and the host
// reads once when the group is decoded.  Finished entry k of window w sits at w B + k.
struct SttBeamBook {
    int32_t *next_tok, *src;         // [R] the row's next input token | the row (of this step) it continues
    float* score;                    // [R] cumulative log-probability of the row's beam
    int32_t *n_live, *n_fin, *done;  // [R], per window: live beams | finished entries | 1 once the finished list is full
    int32_t *fin_step, *fin_beam;    // [R] a finished entry: the step it ended at and the beam (of that step) it extends
    float* fin_score;                // [R]
    int32_t* live;                   // [1] windows of the group still decoding
    int32_t *bp_tok, *bp_par;        // [steps][R] back-pointers: the token a row took at a step and the beam it came from
    // [R] timestamp mode (rt_stt_transcribe_seek) only, a row's history state: bit 0 - its last token is a timestamp, bit 1 - the one
    // before it is (or the history is shorter than two) | the last timestamp id of its history, 0: none.  Written for a next beam from
    // its parent's, so the state follows a beam through `src`
    int32_t *ts_flags, *ts_last;
    int R;
};

// The timestamp rule of a step ("timestamps and seek"): timestamp ids are [t0, t0 + nt), t0 - 1 is
// <|notimestamps|>; max_initial: the largest timestamp index the first generated token may take, -1: no limit
struct SttTsRule { int t0, nt, max_initial; };

// The decoding step rule, stated once for beam search (k_stt_beam_select) and sampled decoding (k_stt_sample_select): which ids a row
// may take at a step, and the normaliser of its log-probabilities over them.  Text ids are [text_lo, text_hi) under the mask (bit 0 of
// a byte bars an id at every step, bit 1 at the first), timestamp ids [ts_lo, ts_hi) whatever the mask says; under TS
// (rt_stt_transcribe_seek) the ranges follow from the row's history state, else there are none and every id the mask leaves is text
struct SttStepIds { int text_lo, text_hi, ts_lo, ts_hi, bad; };
template <bool TS>
__device__ __forceinline__ SttStepIds stt_step_ids(int flags, int lts, int first_step, int eos, int V, const SttTsRule& ts) {
    SttStepIds a{0, 0, 0, 0, first_step ? 3 : 1};
    if constexpr (TS) {
        const bool last = flags & 1, pen = flags & 2;
        a.text_hi = ts.t0 - 1;                                 // <|notimestamps|> never appears
        a.ts_lo = ts.t0; a.ts_hi = min(ts.t0 + ts.nt, V);
        if (lts > 0) a.ts_lo = max(a.ts_lo, (last && !pen) ? lts : lts + 1);      // timestamps do not decrease (nor repeat, outside a pair)
        if (last && pen) a.ts_lo = a.ts_hi;                    // behind a pair (or a lone first timestamp): text
        if (last && !pen) a.text_lo = eos;                     // closing a pair: a timestamp or the end
        if (first_step) {                                      // the first generated token is a timestamp, at most max_initial
            a.text_lo = a.text_hi;
            if (ts.max_initial >= 0) a.ts_hi = min(a.ts_hi, ts.t0 + ts.max_initial + 1);
        }
    }
    return a;
}
// id i with mask byte mk - 0: barred, 1: text, 2: timestamp
template <bool TS>
__device__ __forceinline__ int stt_step_kind(const SttStepIds& a, int i, int mk) {
    if constexpr (TS) {
        if (i >= a.ts_lo && i < a.ts_hi) return 2;
        return (i >= a.text_lo && i < a.text_hi && !(mk & a.bad)) ? 1 : 0;
    } else {
        return (mk & a.bad) ? 0 : 1;
    }
}
// The history state of the row that continues one with (flags, lts) by `tok`
__device__ __forceinline__ void stt_ts_next(int tok, int first_step, int flags, int lts, const SttTsRule& ts, int32_t* flags_out, int32_t* last_out) {
    const bool is_ts = tok >= ts.t0;
    *flags_out = (is_ts ? 1 : 0) | ((first_step || (flags & 1)) ? 2 : 0);
    *last_out = is_ts ? tok : lts;
}

// The normaliser of row x over the ids `a` leaves, by all 1024 threads of a workgroup: the masked maximum, then sum exp(x - max) - per
// thread in index order, butterfly per wave, the 16 wave values (red_v; red_w: the timestamp part) in wave order, so a row's
// log-probabilities do not depend on what else is in the launch, nor on which kernel asks.  A NaN logit takes no part.
// TS: each pass forms the figures of the text part and of the timestamp part side by side (same order of reduction per part);
// timestamps win - every text id is barred, text_ok false - when m_ts + log(s_ts) > m_text, and lse follows from the parts that
// survive.  TS == false: the text part alone, and nothing to decide.
// Every pass over a row (these two, the callers' third) asks for STT_SEL_U logits and mask bytes of the thread at once,
// unconditionally (clamped indices): one round trip per 4 elements instead of one per element behind a per-lane branch (DESIGN.md
// section 9 row 0; 8 would spill at 1024 threads).
struct SttRowNorm { float lse; bool text_ok; };
template <bool TS>
__device__ __forceinline__ SttRowNorm stt_row_norm(const float* __restrict__ x, const uint8_t* __restrict__ mask, int V, const SttStepIds& a,
                                                   float* red_v, float* red_w) {
    const int tid = threadIdx.x, wave = tid >> 6;
    float m = -INFINITY, m2 = -INFINITY;                       // (m2, sum2: the timestamp part, TS only)
    for (int base = tid; base < V; base += 1024 * STT_SEL_U) {
        float xv[STT_SEL_U];
        int mk[STT_SEL_U];
#pragma unroll
        for (int u = 0; u < STT_SEL_U; ++u) { const int i = min(base + 1024 * u, V - 1); xv[u] = x[i]; mk[u] = mask[i]; }
#pragma unroll
        for (int u = 0; u < STT_SEL_U; ++u) {
            const int kd = base + 1024 * u < V ? stt_step_kind<TS>(a, base + 1024 * u, mk[u]) : 0;
            if (kd == 1 && xv[u] > m) m = xv[u];
            if constexpr (TS) { if (kd == 2 && xv[u] > m2) m2 = xv[u]; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((tid & 63) == 0) red_v[wave] = m;
    if constexpr (TS) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m2 = fmaxf(m2, __shfl_xor(m2, o, 64));
        if ((tid & 63) == 0) red_w[wave] = m2;
    }
    __syncthreads();
    m = red_v[0];
    for (int k = 1; k < 16; ++k) m = fmaxf(m, red_v[k]);
    if constexpr (TS) {
        m2 = red_w[0];
        for (int k = 1; k < 16; ++k) m2 = fmaxf(m2, red_w[k]);
    }
    __syncthreads();
    float sum = 0.f, sum2 = 0.f;
    for (int base = tid; base < V; base += 1024 * STT_SEL_U) {
        float xv[STT_SEL_U];
        int mk[STT_SEL_U];
#pragma unroll
        for (int u = 0; u < STT_SEL_U; ++u) { const int i = min(base + 1024 * u, V - 1); xv[u] = x[i]; mk[u] = mask[i]; }
#pragma unroll
        for (int u = 0; u < STT_SEL_U; ++u) {
            const int kd = base + 1024 * u < V ? stt_step_kind<TS>(a, base + 1024 * u, mk[u]) : 0;
            if (kd == 1 && xv[u] == xv[u]) sum += expf(xv[u] - m);
            if constexpr (TS) { if (kd == 2 && xv[u] == xv[u]) sum2 += expf(xv[u] - m2); }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((tid & 63) == 0) red_v[wave] = sum;
    if constexpr (TS) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum2 += __shfl_xor(sum2, o, 64);
        if ((tid & 63) == 0) red_w[wave] = sum2;
    }
    __syncthreads();
    sum = red_v[0];
    for (int k = 1; k < 16; ++k) sum += red_v[k];
    if constexpr (TS) {
        sum2 = red_w[0];
        for (int k = 1; k < 16; ++k) sum2 += red_w[k];
    }
    __syncthreads();
    SttRowNorm n{m + logf(sum), true};
    if constexpr (TS) {
        // the comparison needs no normaliser: logsumexp(timestamps) > max(text) on the raw logits is the same on log-probabilities
        const bool has_ts = m2 > -INFINITY, has_text = m > -INFINITY;
        const float lse_ts = has_ts ? m2 + logf(sum2) : -INFINITY;
        n.text_ok = has_text && !(lse_ts > m);
        if (!n.text_ok) n.lse = lse_ts;
        else if (has_ts) { const float mm = fmaxf(m, m2); n.lse = mm + logf(sum * expf(m - mm) + sum2 * expf(m2 - mm)); }
    }
    return n;
}

// One step of beam search, one workgroup per window.  Per live row: the step rule's ids and normaliser (above), then every thread's
// 9 best (lp, id) in registers, merged through LDS into the row's B + 1 best.  Then wave 0 ranks the window's <= 72 candidates by
// (score descending, beam, id) and thread 0 walks them: end-of-sequence candidates enter the finished list while it has room, the
// others become the next beams until B are taken.  logits row of beam j: w row_stride + j (the step behind the prefix has one row
// per window: row_stride 1, one live beam).  TS (rt_stt_transcribe_seek): the timestamp rule applies, and thread 0 writes a next
// beam's history state from its parent's.
template <bool TS>
__global__ __launch_bounds__(1024) void k_stt_beam_select(const float* __restrict__ logits, int V, int row_stride, const uint8_t* __restrict__ mask,
                                                          int first_step, int eos, int B, int step, SttBeamBook bk, SttTsRule ts) {
    __shared__ float red_v[16];
    __shared__ float red_w[16];
    __shared__ int sh_flags[STT_BEAM_MAX], sh_last[STT_BEAM_MAX];
    __shared__ int red_i[16];
    __shared__ float c_score[STT_BEAM_MAX * STT_CAND];
    __shared__ int c_tok[STT_BEAM_MAX * STT_CAND], c_beam[STT_BEAM_MAX * STT_CAND], c_sorted[STT_BEAM_MAX * STT_CAND];
    const int w = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    if (bk.done[w]) return;                                // (uniform: a completed window rides along untouched)
    const int nl = min(bk.n_live[w], B), K = B + 1;
    if constexpr (TS) {
        if (tid < B) { sh_flags[tid] = bk.ts_flags[w * B + tid]; sh_last[tid] = bk.ts_last[w * B + tid]; }
        __syncthreads();
    }
    for (int j = 0; j < nl; ++j) {
        const float* x = logits + ((int64_t)w * row_stride + j) * V;
        const SttStepIds a = stt_step_ids<TS>(TS ? sh_flags[j] : 0, TS ? sh_last[j] : 0, first_step, eos, V, ts);
        const auto [lse, text_ok] = stt_row_norm<TS>(x, mask, V, a, red_v, red_w);
        float cv[STT_CAND];
        int ci[STT_CAND];
#pragma unroll
        for (int k = 0; k < STT_CAND; ++k) { cv[k] = -INFINITY; ci[k] = STT_NO_ID; }
        for (int base = tid; base < V; base += 1024 * STT_SEL_U) {
            float xv[STT_SEL_U];
            int mk[STT_SEL_U];
#pragma unroll
            for (int u = 0; u < STT_SEL_U; ++u) { const int i = min(base + 1024 * u, V - 1); xv[u] = x[i]; mk[u] = mask[i]; }
#pragma unroll
            for (int u = 0; u < STT_SEL_U; ++u) {
                const int i = base + 1024 * u;
                const float lp = xv[u] - lse;
                const int kd = i < V ? stt_step_kind<TS>(a, i, mk[u]) : 0;
                if (kd == 0 || (kd == 1 && !text_ok)) continue;
                if (!(lp == lp) || !cand_before(lp, i, cv[STT_CAND - 1], ci[STT_CAND - 1])) continue;
                cv[STT_CAND - 1] = lp; ci[STT_CAND - 1] = i;
#pragma unroll
                for (int k = STT_CAND - 1; k > 0; --k)
                    if (cand_before(cv[k], ci[k], cv[k - 1], ci[k - 1])) {
                        const float tv = cv[k]; cv[k] = cv[k - 1]; cv[k - 1] = tv;
                        const int ti = ci[k]; ci[k] = ci[k - 1]; ci[k - 1] = ti;
                    }
            }
        }
        const float s_j = bk.score[w * B + j];
        for (int r = 0; r < K; ++r) {
            float bv = cv[0];
            int bi = ci[0];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (cand_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if ((tid & 63) == 0) { red_v[wave] = bv; red_i[wave] = bi; }
            __syncthreads();
            bv = red_v[0]; bi = red_i[0];
            for (int k = 1; k < 16; ++k)
                if (cand_before(red_v[k], red_i[k], bv, bi)) { bv = red_v[k]; bi = red_i[k]; }
            if (bi != STT_NO_ID && bi == ci[0]) {            // the winner's owner (ids are unique in a row) drops it
#pragma unroll
                for (int k = 0; k + 1 < STT_CAND; ++k) { cv[k] = cv[k + 1]; ci[k] = ci[k + 1]; }
                cv[STT_CAND - 1] = -INFINITY; ci[STT_CAND - 1] = STT_NO_ID;
            }
            if (tid == 0) {
                const bool some = bi != STT_NO_ID && bv > -INFINITY;
                c_score[j * K + r] = some ? s_j + bv : -INFINITY;
                c_tok[j * K + r] = bi;
                c_beam[j * K + r] = j;
            }
            __syncthreads();
        }
    }
    const int n = nl * K;
    if (wave == 0)
        for (int c = tid; c < n; c += 64) {
            int rank = 0;
            for (int o = 0; o < n; ++o) {
                const bool before = c_score[o] > c_score[c] ||
                                    (c_score[o] == c_score[c] && (c_beam[o] < c_beam[c] || (c_beam[o] == c_beam[c] && (c_tok[o] < c_tok[c] || (c_tok[o] == c_tok[c] && o < c)))));
                rank += before ? 1 : 0;
            }
            c_sorted[rank] = c;
        }
    __syncthreads();
    if (tid != 0) return;
    int nb = 0, nf = bk.n_fin[w];
    for (int c = 0; c < n && nb < B; ++c) {
        const int id = c_sorted[c];
        const float sc = c_score[id];
        if (!(sc > -INFINITY)) break;                      // (behind the last candidate a row could offer)
        if (c_tok[id] == eos) {
            if (nf < B) { bk.fin_step[w * B + nf] = step; bk.fin_beam[w * B + nf] = c_beam[id]; bk.fin_score[w * B + nf] = sc; ++nf; }
        } else {
            const int row = w * B + nb;
            bk.next_tok[row] = c_tok[id];
            bk.src[row] = w * B + c_beam[id];
            bk.score[row] = sc;
            bk.bp_tok[(int64_t)step * bk.R + row] = c_tok[id];
            bk.bp_par[(int64_t)step * bk.R + row] = c_beam[id];
            if constexpr (TS) stt_ts_next(c_tok[id], first_step, sh_flags[c_beam[id]], sh_last[c_beam[id]], ts, &bk.ts_flags[row], &bk.ts_last[row]);
            ++nb;
        }
    }
    for (int i = nb; i < B; ++i) bk.src[w * B + i] = w * B + i;     // rows without a beam continue themselves (nothing reads them)
    bk.n_fin[w] = nf;
    bk.n_live[w] = nb;
    if (nf >= B || nb == 0) {
        bk.done[w] = 1;
        atomicSub(bk.live, 1);
    }
}

// ---------------------------------------------------------------------------------------------- sampled decoding (temperature fallback)
// The generator of a sampled step ("temperature fallback"): the mix32 chain of rt_uniform (sampling.hip) over
// (seed, window key, temperature index, sample index, step) per row and the id per element.  The top 23 bits of the hash are k;
// u = (k + 0.5) 2^-23 is exact in float32 and lies in [2^-24, 1 - 2^-24], so g = -log(-log(u)) is finite.
__device__ __forceinline__ unsigned stt_mix32(unsigned h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__device__ __forceinline__ unsigned stt_gumbel_row(unsigned seed_lo, unsigned seed_hi, unsigned key, unsigned t_index, unsigned sample, unsigned step) {
    const unsigned a = stt_mix32(seed_lo ^ 0x85EBCA6Bu);
    const unsigned b = stt_mix32(a + key * 0x9E3779B1u);
    const unsigned c = stt_mix32(b + t_index * 0x85EBCA77u);
    const unsigned d = stt_mix32(c + sample * 0xC2B2AE3Du + seed_hi);
    return stt_mix32(d + step * 0x9E3779B1u);
}
__device__ __forceinline__ float stt_gumbel(unsigned row_hash, int id) {
    const unsigned k = stt_mix32(row_hash + (unsigned)id * 0x85EBCA77u) >> 9;
    const float u = __fmul_rn(__fadd_rn((float)k, 0.5f), 1.0f / 8388608.0f);
    return -logf(-logf(u));
}

// What a sampled step takes beside the step rule: the temperature (> 0), the seed, the temperature's index in the policy, and per
// row the window key and the sample index (a row's pick depends on these and its logits alone, not on where it sits in a launch)
struct SttSampleRule { float T; unsigned seed_lo, seed_hi, t_index; const int32_t* key; const int32_t* sample; };

// One sampled step, one workgroup per ROW (window x sample; row w S + j is sample j of window w, its logits at row
// w row_stride + (row_stride > 1 ? j : 0): the step behind the prefix has one row of logits per window).  The step rule (the
// functions k_stt_beam_select calls) on the UNTEMPERED logits gives the row's log-probabilities and the decision "timestamps win";
// one more pass takes the arg-max of x / T + g(id) over the surviving ids (Gumbel-max: the pick is distributed as softmax(x / T)
// over them), the lower id on ties.  A NaN or -inf logit takes no part.  The row's score adds the untempered log-probability of the
// pick; end-of-sequence (or a row without any survivor, which counts as ending) sets the row's done flag and takes it out of `live`;
// a row that is done rides along untouched.
// src: the row itself, and behind the prefix the window's first row, whose cache slot the prefix pass wrote.  win_val (tests, else
// null): the winning perturbed value per row.
template <bool TS>
__global__ __launch_bounds__(1024) void k_stt_sample_select(const float* __restrict__ logits, int V, int row_stride, const uint8_t* __restrict__ mask,
                                                            int first_step, int eos, int S, int step, SttBeamBook bk, SttTsRule ts, SttSampleRule sr,
                                                            float* __restrict__ win_val) {
    __shared__ float red_v[16];
    __shared__ float red_w[16];
    __shared__ int red_i[16];
    const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    if (bk.done[r]) return;                                // (uniform)
    const int w = r / S, j = r - w * S;
    const float* x = logits + ((int64_t)w * row_stride + (row_stride > 1 ? j : 0)) * V;
    int flags = 0, lts = 0;
    if constexpr (TS) { flags = bk.ts_flags[r]; lts = bk.ts_last[r]; }      // (thread 0 writes them behind the last barrier)
    const SttStepIds a = stt_step_ids<TS>(flags, lts, first_step, eos, V, ts);
    const auto [lse, text_ok] = stt_row_norm<TS>(x, mask, V, a, red_v, red_w);
    // the arg-max of x / T + g over the survivors
    const unsigned row_hash = stt_gumbel_row(sr.seed_lo, sr.seed_hi, (unsigned)sr.key[r], sr.t_index, (unsigned)sr.sample[r], (unsigned)step);
    float bv = -INFINITY;
    int bi = STT_NO_ID;
    for (int base = tid; base < V; base += 1024 * STT_SEL_U) {
        float xv[STT_SEL_U];
        int mk[STT_SEL_U];
#pragma unroll
        for (int u = 0; u < STT_SEL_U; ++u) { const int i = min(base + 1024 * u, V - 1); xv[u] = x[i]; mk[u] = mask[i]; }
#pragma unroll
        for (int u = 0; u < STT_SEL_U; ++u) {
            const int i = base + 1024 * u;
            const int kd = i < V ? stt_step_kind<TS>(a, i, mk[u]) : 0;
            if (kd == 0 || (kd == 1 && !text_ok)) continue;
            const float v = __fadd_rn(__fdiv_rn(xv[u], sr.T), stt_gumbel(row_hash, i));
            if (v > -INFINITY && cand_before(v, i, bv, bi)) { bv = v; bi = i; }      // (a NaN compares false)
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (cand_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { red_v[wave] = bv; red_i[wave] = bi; }
    __syncthreads();
    if (tid != 0) return;
    bv = red_v[0]; bi = red_i[0];
    for (int k = 1; k < 16; ++k)
        if (cand_before(red_v[k], red_i[k], bv, bi)) { bv = red_v[k]; bi = red_i[k]; }
    const bool some = bi != STT_NO_ID;
    const int tok = some ? bi : eos;
    bk.next_tok[r] = tok;
    bk.src[r] = row_stride > 1 ? r : w * S;
    if (some) bk.score[r] = bk.score[r] + (x[bi] - lse);
    bk.bp_tok[(int64_t)step * bk.R + r] = tok;
    bk.bp_par[(int64_t)step * bk.R + r] = j;
    if (win_val) win_val[r] = bv;
    if constexpr (TS) stt_ts_next(tok, first_step, flags, lts, ts, &bk.ts_flags[r], &bk.ts_last[r]);
    if (tok == eos) {
        bk.done[r] = 1;
        atomicSub(bk.live, 1);
    }
}

// The four planes of a decoder self-attention cache
struct SttKvPlanes { const bf16_t* src[4]; bf16_t* dst[4]; };
// Row r of the next step continues row src[r] of this one: positions [0, len) of every (layer, head) of cache slot src[r] are
// copied into slot r of the OTHER cache (two rows may swap parents, and two children of one parent diverge at the next position).
// blockIdx = (head, row, layer); a copy is len x head_dim contiguous bf16, moved 16 bytes per thread.
__global__ __launch_bounds__(256) void k_stt_beam_reorder(SttKvPlanes p, const int32_t* __restrict__ src, int slots, int heads, int max_pos, int head_dim, int len) {
    const int h = blockIdx.x, r = blockIdx.y, l = blockIdx.z;
    const int from = src[r];
    if (from < 0 || from >= slots) return;
    const int64_t per = (int64_t)max_pos * head_dim;
    const int64_t a = (((int64_t)l * slots + from) * heads + h) * per, b = (((int64_t)l * slots + r) * heads + h) * per;
    const int n16 = len * head_dim / 8;                    // (head_dim is a multiple of 32)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4* s4 = (const uint4*)(p.src[q] + a);
        uint4* d4 = (uint4*)(p.dst[q] + b);
        for (int i = threadIdx.x; i < n16; i += 256) d4[i] = s4[i];
    }
}

// rows of the beam path's prefix pass (row w per + i: the window's first beam row as its cache slot, position i, window w) and of its
// step passes (row r: its own slot, window r / B)
__global__ void k_stt_fill_beam_rows(int32_t* __restrict__ pre_slot, int32_t* __restrict__ pre_pos, int32_t* __restrict__ pre_win, int n_pre, int per, int B,
                                     int32_t* __restrict__ row_slot, int32_t* __restrict__ row_win, int n_rows) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < max(n_pre, n_rows); i += gridDim.x * blockDim.x) {
        if (i < n_pre) { pre_slot[i] = i / per * B; pre_pos[i] = i % per; pre_win[i] = i / per; }
        if (i < n_rows) { row_slot[i] = i; row_win[i] = i / B; }
    }
}

// ---------------------------------------------------------------------------------------------- conditioning on previous text (rt_stt_set_prompt)
// The kernels of a prompt policy ("conditioning on previous text"): windows of one group decode behind prefixes
// of different lengths, so every row of a pass takes its position from a table the host laid out and proved in range.
//
// x[r][:] = token_embedding[tok[r]] + position_embedding[pos[r]]: k_stt_embed with the row's position read from a table
__global__ void k_stt_embed_rows(const bf16_t* __restrict__ tok_emb, const float* __restrict__ pos_emb, const int32_t* __restrict__ tok,
                                 const int32_t* __restrict__ pos, int D, float* __restrict__ x) {
    const int r = blockIdx.x;
    const int64_t t = tok[r], at = pos[r];
    for (int i = threadIdx.x; i < D; i += blockDim.x) x[(int64_t)r * D + i] = bf16_to_f32(tok_emb[t * D + i]) + pos_emb[at * D + i];
}
// The tokens of a ragged prefix pass: the host lays a window's prompt ids out as they are and writes -(1 + k) where entry k of the
// window's forced prefix goes - the device may have decided its language (k_stt_lang_prefix) - which this kernel fills in
__global__ void k_stt_prompt_tokens(int32_t* __restrict__ tok, const int32_t* __restrict__ win, int n, const int32_t* __restrict__ win_prefix, int P) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int t = tok[i];
        const int forced = win_prefix[win[i] * P + min(max(-t - 1, 0), P - 1)];      // (asked for whatever t is: no load behind a per-lane branch)
        tok[i] = t < 0 ? forced : t;
    }
}
// out[w][:] = x[rows[w]][:]: the last prefix row of every window, dense, for the final LayerNorm (D is a multiple of 8)
__global__ void k_stt_take_rows(const float* __restrict__ x, const int32_t* __restrict__ rows, int D, float* __restrict__ out) {
    const float4* s4 = (const float4*)(x + (int64_t)rows[blockIdx.x] * D);
    float4* d4 = (float4*)(out + (int64_t)blockIdx.x * D);
    for (int i = threadIdx.x; i < D / 4; i += blockDim.x) d4[i] = s4[i];
}
// k_stt_beam_reorder with a range per row: positions [lo[r], hi[r]) of slot src[r] go to slot r of the other cache (skip_self: the
// two caches are one, and a row that continues itself has nothing to move).  The prefix of a window never diverges between its rows,
// so it is written into both caches once and the gather between steps moves the generated positions alone.
__global__ __launch_bounds__(256) void k_stt_beam_reorder_range(SttKvPlanes p, const int32_t* __restrict__ src, const int32_t* __restrict__ lo,
                                                                const int32_t* __restrict__ hi, int slots, int heads, int max_pos, int head_dim, int skip_self) {
    const int h = blockIdx.x, r = blockIdx.y, l = blockIdx.z;
    const int from = src[r], a0 = max(lo[r], 0), a1 = min(hi[r], max_pos);
    if (from < 0 || from >= slots || a1 <= a0 || (skip_self && from == r)) return;
    const int64_t per = (int64_t)max_pos * head_dim;
    const int64_t a = (((int64_t)l * slots + from) * heads + h) * per + (int64_t)a0 * head_dim;
    const int64_t b = (((int64_t)l * slots + r) * heads + h) * per + (int64_t)a0 * head_dim;
    const int n16 = (a1 - a0) * head_dim / 8;              // (head_dim is a multiple of 32)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4* s4 = (const uint4*)(p.src[q] + a);
        uint4* d4 = (uint4*)(p.dst[q] + b);
        for (int i = threadIdx.x; i < n16; i += 256) d4[i] = s4[i];
    }
}
// A unit (a window of the beam path, a row of the sampled path) whose budget is `step` stops: its done flag is set and it leaves
// `live`, as if it had ended - the select kernels then pass it by, and the host offers what it holds to the ranker
__global__ void k_stt_retire(int32_t* __restrict__ done, int32_t* __restrict__ live, const int32_t* __restrict__ budget, int n, int step) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n && budget[k] == step && !done[k]) { done[k] = 1; atomicSub(live, 1); }
}

}  // namespace

// Windows of one group: the rows of every launch.  Compile-time: the group's buffers - about 79 MB per window at Whisper-tiny
// dimensions - are the price of a larger group.
constexpr int STT_GROUP = 32;

// The workspaces of one pre-LN layer over some rows (stt_layer): [rows][D], qkv [rows][3 D], ff [rows][ffn]
struct SttWork { float *x = nullptr, *xn = nullptr, *qkv = nullptr, *q = nullptr, *ao = nullptr, *ff = nullptr; };

// The encoder side of a group of B windows: front end, encoder, and the cross-attention cache the decoders read.  Row tables address
// the caches per row: encoder row b n_ctx + t is position t of slot b and attends up to n_ctx - 1.
struct SttEnc {
    KvCache kv, cross_kv;
    float *pcm16k = nullptr, *mel = nullptr, *c1 = nullptr, *out = nullptr;     // out: the encoder states [B][n_ctx][D]
    SttWork work;
    int32_t *slot = nullptr, *pos = nullptr, *last = nullptr;                   // [B n_ctx] (last: n_ctx - 1 throughout)
    int32_t* d_gmax = nullptr;
    SttWin* d_wins = nullptr;
};

// A decoder side for `rows` rows (greedy: the windows of a group; beam search: windows x beams): the self-attention cache, one slot
// per row, workspaces for rows x n_prefix rows of a pass, the logits of every row's last position and the tokens a pass reads.
struct SttDec {
    KvCache kv;
    SttWork work;
    float* logits = nullptr;            // [rows][vocab]
    int32_t* enc_last = nullptr;        // [rows n_prefix] n_ctx - 1 throughout: how far a row attends across the encoder states
    const int32_t* tok = nullptr;       // the tokens of the next pass (not owned)
};

// The one buffer set of the handle: B windows' encoder side and their greedy decoder side, reserved for one window by
// rt_stt_finalize and replaced by a larger set when a call needs more windows (stt_group_reserve).
struct SttGroup {
    int B = 0;
    SttEnc enc;
    SttDec dec;
    int32_t *pre_slot = nullptr, *pre_pos = nullptr;       // [B n_prefix] rows of the prefix pass: row b n_prefix + i -> slot b, position i
    int32_t *step_slot = nullptr, *step_pos = nullptr;     // [B] rows of a step pass: slot b, position 0 (+ pos_add)
    int32_t *d_prefix = nullptr, *d_tok = nullptr;         // [B n_prefix] the forced prefix of every window | [B] every row's pick (k_stt_pick)
    std::vector<void*> owned;
};

// The beam path (rt_stt_transcribe_beam), for `rows` rows = windows x beams of one group: a decoder side, a second self-attention
// cache (k_stt_beam_reorder gathers from dec.kv into it, then the two swap), row tables and the bookkeeping of k_stt_beam_select.
// The encoder side and the cross-attention cache are the group's (s->grp.enc).
struct SttBeam {
    int rows = 0;
    SttDec dec;
    KvCache kv_next;
    int32_t *pre_slot = nullptr, *pre_pos = nullptr, *pre_win = nullptr;                       // [rows n_prefix] the prefix pass
    int32_t *row_slot = nullptr, *row_win = nullptr, *row_pos = nullptr;                       // [rows] a step pass
    int32_t* book_mem = nullptr;
    size_t book_n = 0;
    SttBeamBook book{};
    // sampled decoding (stt_decode_sample_group): the row tables of a subset of the group's windows, their prefixes, and the rows'
    // keys and sample indices, uploaded per attempt in one copy: [rows n_prefix] x 4 (pre_slot | pre_pos | pre_win | prefix), [rows] x 4
    // (row_slot | row_win | key | sample)
    int32_t* smp = nullptr;
    std::vector<void*> owned;
};

// The device side of a prompt policy (rt_stt_set_prompt), for groups of `wins` windows and `rows` decoder rows: the workspaces of the
// ragged prefix pass - one row per prefix token of every window, at most max_prefix each - and the tables of one decode.  Nothing of
// it exists until a policy is first used; it grows with the group as the beam path's set does.  The existing sets are not enlarged.
struct SttPrompt {
    int wins = 0, rows = 0;
    SttWork work;                       // [wins max_prefix] rows
    float* xlast = nullptr;             // [wins][D] every window's last prefix row, dense
    int32_t* enc_last = nullptr;        // [wins max_prefix] n_ctx - 1 throughout
    int32_t* tab = nullptr;             // the tables of one decode (SttPrTab), uploaded in one copy
    size_t tab_n = 0;
    std::vector<void*> owned;
};
// The tables of one decode under a prompt policy, as offsets into SttPrompt::tab (and into the host copy they are laid out in).  M
// rows of the prefix pass: cache slot of the window's first decoder row, position, window of the group, token (-(1 + k): entry k of
// the window's forced prefix, k_stt_prompt_tokens).  Per window: its last prefix row and its budget.  Per decoder row: its budget,
// its prefix length, zero, its window's first row; per step and row: the position the step's pass writes and the end of the range
// the gather before it moves, both clamped to what the row's budget allows - a window whose budget is spent rides along in place.
struct SttPrTab {
    int M = 0, nW = 0, rows = 0, steps = 0, longest = 0;      // steps: the largest budget of the group; longest: its longest prefix
    size_t pre_slot = 0, pre_pos = 0, pre_win = 0, pre_tok = 0, last_row = 0, win_budget = 0, row_budget = 0, base = 0, zero = 0, fan_src = 0, step_pos = 0,
           step_hi = 0, total = 0;
    std::vector<char> retire_win, retire_row;    // [steps + 1] a window / a row has this budget, below the largest
};

// One window's line of rt_stt_fallback_report
struct SttFbWin { int32_t attempts = 1; float temperature = 0.f, ratio = NAN; };

// What stt_layer takes to write cross-attention probabilities out (rt_stt_align): the alignment rows of the pass, per decoder layer its
// alignment heads, and W[window][head][row][F_max] with the stride between two heads of a window
struct SttCapture { AlignRows rows; int n_rows; const AlignHeads* per_layer; int64_t head_stride; float* W; };

// The device side of rt_stt_align (nothing of it exists until the first call; replaced by a larger set when a group needs more, as the
// beam path's set): workspaces for the rows of the teacher-forced pass, a chunk of logits, W, M, the path kernel's outputs and scratch,
// and the tables of one group, uploaded in one copy
constexpr int STT_ALIGN_CHUNK = 256;    // rows of logits formed at a time
struct SttAlignNeed { size_t rows = 0, w = 0, m = 0, stats = 0, trace = 0, tab = 0, arows = 0; };
struct SttAlignBuf {
    SttAlignNeed has;
    SttWork work;                       // [rows]
    int32_t* enc_last = nullptr;        // [rows] n_ctx - 1 throughout
    float *xl = nullptr, *xn = nullptr, *logits = nullptr;     // [STT_ALIGN_CHUNK] rows: taken, normed, their logits
    float *W = nullptr, *M = nullptr, *lp = nullptr;           // lp [arows]
    double* stats = nullptr;
    uint32_t* trace = nullptr;
    int32_t *frames = nullptr, *tab = nullptr;                 // frames [arows]
    std::vector<void*> owned;
};

struct rt_stt {
    rt_ctx* ctx = nullptr;
    rt_stt_config cfg{};
    std::vector<SttSlot> slots;
    std::map<std::string, int> by_name;
    bool finalized = false;
    // front-end constants
    double *d_twc = nullptr, *d_tws = nullptr;
    float *d_window = nullptr, *d_melT = nullptr;
    Resampler rs;                     // polyphase filter of the last (sr_in -> cfg.sample_rate) pair (resample.h)
    SttGroup grp;                     // every entry point's buffers: one window from rt_stt_finalize on
    SttBeam beam;                     // the beam path: nothing of it exists until the first rt_stt_transcribe_beam
    std::vector<int32_t> h_book;
    std::vector<SttWin> h_wins;       // host copies of what is uploaded per group (alive until the group's last synchronisation)
    std::vector<int32_t> h_tok;
    uint8_t* d_mask = nullptr;
    std::vector<int32_t> suppress_ids;   // rt_stt_set_suppress: ids never produced (a generation config's `suppress_tokens`)
    // rt_stt_set_languages: the ids position 1 of the prefix may take and the no-speech id; the device side (one group's worth,
    // allocated by rt_stt_finalize) of the probe pass, k_stt_probe and k_stt_lang_prefix
    std::vector<int32_t> lang_ids;
    int32_t no_speech_id = -1;
    int32_t* d_lang_ids = nullptr;
    int32_t* d_sot = nullptr;            // [STT_GROUP] start-of-transcript: the tokens of the probe pass
    int32_t* d_probe = nullptr;          // [4][STT_GROUP]: detected id | its probability | no-speech probability (float) | the id the prefix took
    int32_t* d_win_meta = nullptr;       // [2][STT_GROUP]: a window's clip | the row of its clip's first window in this group (-1: none)
    int32_t* d_clip_lang = nullptr;      // [clip_lang_cap] per clip of the call: the forced or detected id, -1 until it is detected
    int clip_lang_cap = 0;
    std::vector<int32_t> h_probe, h_meta;
    // rt_stt_set_timestamps: timestamp ids [ts_begin, ts_begin + ts_count), 0: not configured (rt_stt_transcribe_seek refuses)
    int32_t ts_begin = 0, ts_count = 0;
    // [STT_GROUP][n_prefix] a prefix per window (SttPlan; in timestamp mode n_prefix - 1 entries each, without <|notimestamps|>):
    // allocated by rt_stt_finalize for a handle with languages or timestamps
    int32_t* d_win_prefix = nullptr;
    // rt_stt_set_fallback: the policy (fb_set: one is set) and, per window of the last call under it, what rt_stt_fallback_report returns
    bool fb_set = false;
    rt_stt_fallback fb{};
    std::vector<SttFbWin> fb_report;
    std::vector<int32_t> h_smp;
    // rt_stt_set_prompt: the policy (pr_set: one is set; pr_initial: the copy of its initial prompt), its device side, the tables of the
    // decode in flight with their host copy, and per window of the last seek call what rt_stt_prompt_report returns
    bool pr_set = false;
    rt_stt_prompt pr{};
    std::vector<int32_t> pr_initial;
    SttPrompt prm;
    SttPrTab pr_tab;
    std::vector<int32_t> h_prm;
    std::vector<std::pair<int32_t, int32_t>> pr_report;      // (prompt length, the reset mark moved behind the window)
    // rt_stt_set_alignment: the alignment heads as (decoder layer, head) in the caller's order (empty: rt_stt_align refuses), the same
    // per layer, the median width; the device side and the host copies of what a group uploads and reads back
    std::vector<std::pair<int32_t, int32_t>> al_heads;
    std::vector<AlignHeads> al_layers;
    int32_t al_width = 0;
    SttAlignBuf aln;
    std::vector<int32_t> h_aln, h_aln_frames;
    std::vector<float> h_aln_lp;
    // rt_debug_stt_align_timing: events around the launches rt_stt_align adds (0: the capture launches, 1: statistics + matrix, 2: the
    // paths), summed per class when a group has synchronised
    bool al_clock = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> al_events[3];
    double al_ms[3] = {0.0, 0.0, 0.0};
    std::vector<void*> owned;
};

namespace {

void stt_slot(rt_stt* s, const std::string& name, int kind, int64_t rows, int64_t cols) {
    SttSlot sl;
    sl.name = name; sl.kind = kind; sl.rows = rows; sl.cols = cols;
    s->by_name[name] = (int)s->slots.size();
    s->slots.push_back(sl);
}
SttSlot* stt_find(rt_stt* s, const std::string& n) {
    auto it = s->by_name.find(n);
    return it == s->by_name.end() ? nullptr : &s->slots[it->second];
}
const PackedW& SPW(rt_stt* s, const std::string& n) { return stt_find(s, n)->pw; }
float* SVEC(rt_stt* s, const std::string& n) { return stt_find(s, n)->vec; }

void stt_declare(rt_stt* s) {
    const rt_stt_config& c = s->cfg;
    const int D = c.d_model, F = c.ffn;
    stt_slot(s, "enc.conv1", S_GEMM, D, 3 * (int64_t)c.n_mels);          // [Co][tap * Ci + ci]
    stt_slot(s, "enc.conv1_b", S_VEC, D, 1);
    stt_slot(s, "enc.conv2", S_GEMM, D, 4 * (int64_t)D);                  // stride-2 k3 conv as a 2-tap GEMM over [T/2][2 D] rows
    stt_slot(s, "enc.conv2_b", S_VEC, D, 1);
    stt_slot(s, "enc.pos", S_VEC, (int64_t)c.n_ctx * D, 1);
    auto layer = [&](const std::string& p, bool cross) {
        stt_slot(s, p + ".ln1_w", S_VEC, D, 1); stt_slot(s, p + ".ln1_b", S_VEC, D, 1);
        stt_slot(s, p + ".wqkv", S_GEMM, 3 * (int64_t)D, D); stt_slot(s, p + ".bqkv", S_VEC, 3 * (int64_t)D, 1);
        stt_slot(s, p + ".wo", S_GEMM, D, D); stt_slot(s, p + ".bo", S_VEC, D, 1);
        if (cross) {
            stt_slot(s, p + ".lnc_w", S_VEC, D, 1); stt_slot(s, p + ".lnc_b", S_VEC, D, 1);
            stt_slot(s, p + ".cwq", S_GEMM, D, D); stt_slot(s, p + ".cbq", S_VEC, D, 1);
            stt_slot(s, p + ".cwkv", S_GEMM, 2 * (int64_t)D, D); stt_slot(s, p + ".cbkv", S_VEC, 2 * (int64_t)D, 1);
            stt_slot(s, p + ".cwo", S_GEMM, D, D); stt_slot(s, p + ".cbo", S_VEC, D, 1);
        }
        stt_slot(s, p + ".ln2_w", S_VEC, D, 1); stt_slot(s, p + ".ln2_b", S_VEC, D, 1);
        stt_slot(s, p + ".fc1", S_GEMM, F, D); stt_slot(s, p + ".fc1_b", S_VEC, F, 1);
        stt_slot(s, p + ".fc2", S_GEMM, D, F); stt_slot(s, p + ".fc2_b", S_VEC, D, 1);
    };
    for (int i = 0; i < c.enc_layers; ++i) layer("enc.l" + std::to_string(i), false);
    stt_slot(s, "enc.ln_w", S_VEC, D, 1); stt_slot(s, "enc.ln_b", S_VEC, D, 1);
    stt_slot(s, "dec.tok", S_TABLE, c.vocab, D);                          // token embedding = tied LM head
    stt_slot(s, "dec.pos", S_VEC, (int64_t)c.n_text_ctx * D, 1);
    for (int i = 0; i < c.dec_layers; ++i) layer("dec.l" + std::to_string(i), true);
    stt_slot(s, "dec.ln_w", S_VEC, D, 1); stt_slot(s, "dec.ln_b", S_VEC, D, 1);
    stt_slot(s, "fe.window", S_VEC, c.n_fft, 1);
    stt_slot(s, "fe.melT", S_VEC, (int64_t)(c.n_fft / 2 + 1) * c.n_mels, 1);   // [bins][mels]
}

template <typename T>
int stt_alloc(rt_stt* s, std::vector<void*>& owned, size_t n, T** out) {
    void* p = nullptr;
    RT_HIP(s->ctx, hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
    owned.push_back(p);
    *out = (T*)p;
    return RT_OK;
}

int stt_kv(rt_stt* s, std::vector<void*>& owned, KvCache& kv, int layers, int slots, int max_pos) {
    const rt_stt_config& c = s->cfg;
    kv.layers = layers; kv.slots = slots; kv.kv_heads = c.heads; kv.max_pos = max_pos; kv.head_dim = c.d_model / c.heads;
    const size_t n = (size_t)layers * kv.layer_stride();
    RT_TRY(stt_alloc(s, owned, n, &kv.k)); RT_TRY(stt_alloc(s, owned, n, &kv.v)); RT_TRY(stt_alloc(s, owned, n, &kv.k_lo)); RT_TRY(stt_alloc(s, owned, n, &kv.v_lo));
    for (bf16_t* p : {kv.k, kv.v, kv.k_lo, kv.v_lo}) RT_HIP(s->ctx, hipMemsetAsync(p, 0, n * sizeof(bf16_t), s->ctx->stream));
    return RT_OK;
}

int stt_alloc_work(rt_stt* s, std::vector<void*>& owned, size_t rows, SttWork& k) {
    const size_t D = s->cfg.d_model;
    RT_TRY(stt_alloc(s, owned, rows * D, &k.x)); RT_TRY(stt_alloc(s, owned, rows * D, &k.xn)); RT_TRY(stt_alloc(s, owned, rows * 3 * D, &k.qkv));
    RT_TRY(stt_alloc(s, owned, rows * D, &k.q)); RT_TRY(stt_alloc(s, owned, rows * D, &k.ao)); RT_TRY(stt_alloc(s, owned, rows * s->cfg.ffn, &k.ff));
    return RT_OK;
}

// a decoder side for `rows` rows; a pass runs at most n_prefix rows of each (the forced prefix, then one)
int stt_alloc_dec(rt_stt* s, std::vector<void*>& owned, int rows, SttDec& d) {
    const rt_stt_config& c = s->cfg;
    const size_t rp = (size_t)rows * c.n_prefix;
    RT_TRY(stt_kv(s, owned, d.kv, c.dec_layers, rows, c.n_text_ctx));
    RT_TRY(stt_alloc_work(s, owned, rp, d.work));
    RT_TRY(stt_alloc(s, owned, (size_t)rows * c.vocab, &d.logits));
    RT_TRY(stt_alloc(s, owned, rp, &d.enc_last));
    hipLaunchKernelGGL(k_stt_fill_i32, dim3(1), dim3(256), 0, s->ctx->stream, d.enc_last, (int)rp, c.n_ctx - 1, 0);
    RT_HIP(s->ctx, hipGetLastError());
    return RT_OK;
}

// the buffer set of B windows
int stt_alloc_group(rt_stt* s, SttGroup& w, int B) {
    rt_ctx* ctx = s->ctx;
    const rt_stt_config& c = s->cfg;
    const int D = c.d_model, T = c.n_ctx, T2 = 2 * T, P = c.n_prefix;
    const size_t b = (size_t)B, rows = b * T, r = b * P;
    SttEnc& e = w.enc;
    RT_TRY(stt_kv(s, w.owned, e.kv, c.enc_layers, B, T));
    RT_TRY(stt_kv(s, w.owned, e.cross_kv, c.dec_layers, B, T));
    RT_TRY(stt_alloc(s, w.owned, b * c.chunk_seconds * c.sample_rate, &e.pcm16k));
    RT_TRY(stt_alloc(s, w.owned, b * T2 * c.n_mels, &e.mel));
    RT_TRY(stt_alloc(s, w.owned, b * T2 * D, &e.c1));
    RT_TRY(stt_alloc_work(s, w.owned, rows, e.work));
    RT_TRY(stt_alloc(s, w.owned, rows * D, &e.out));
    RT_TRY(stt_alloc(s, w.owned, rows, &e.slot)); RT_TRY(stt_alloc(s, w.owned, rows, &e.pos)); RT_TRY(stt_alloc(s, w.owned, rows, &e.last));
    RT_TRY(stt_alloc(s, w.owned, b, &e.d_gmax)); RT_TRY(stt_alloc(s, w.owned, b, &e.d_wins));
    RT_TRY(stt_alloc_dec(s, w.owned, B, w.dec));
    RT_TRY(stt_alloc(s, w.owned, r, &w.pre_slot)); RT_TRY(stt_alloc(s, w.owned, r, &w.pre_pos));
    RT_TRY(stt_alloc(s, w.owned, b, &w.step_slot)); RT_TRY(stt_alloc(s, w.owned, b, &w.step_pos));
    RT_TRY(stt_alloc(s, w.owned, r, &w.d_prefix)); RT_TRY(stt_alloc(s, w.owned, b, &w.d_tok));
    std::vector<int32_t> prefix(r);
    for (size_t i = 0; i < r; ++i) prefix[i] = c.prefix[i % P];
    RT_HIP(ctx, hipMemcpy(w.d_prefix, prefix.data(), r * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_stt_fill_rows, dim3(64), dim3(256), 0, ctx->stream, e.slot, e.pos, (int)rows, T);
    hipLaunchKernelGGL(k_stt_fill_i32, dim3(64), dim3(256), 0, ctx->stream, e.last, (int)rows, T - 1, 0);
    hipLaunchKernelGGL(k_stt_fill_rows, dim3(1), dim3(256), 0, ctx->stream, w.pre_slot, w.pre_pos, (int)r, P);
    hipLaunchKernelGGL(k_stt_fill_i32, dim3(1), dim3(64), 0, ctx->stream, w.step_slot, B, 0, 1);
    hipLaunchKernelGGL(k_stt_fill_i32, dim3(1), dim3(64), 0, ctx->stream, w.step_pos, B, 0, 0);
    RT_HIP(ctx, hipGetLastError());
    w.B = B;
    return RT_OK;
}

// Replaces the buffer set `held` (an SttGroup or an SttBeam) by what `build` allocates.  The new set is built aside and adopted only
// when every allocation has succeeded; after a failure (a full group is 2.5 GB beside the TTS model) the handle holds no set at all -
// every pointer null - and the next call allocates again.
template <typename Set, typename Build>
int stt_reserve(rt_stt* s, Set& held, Build build) {
    rt_ctx* ctx = s->ctx;
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (void* p : held.owned) (void)hipFree(p);
    held = Set{};
    Set nw;
    const int rc = build(nw);
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);         // (the fills and memsets already launched on the partial set)
        for (void* p : nw.owned) (void)hipFree(p);
        (void)hipGetLastError();                         // (the failed call's sticky error must not surface at a later launch check)
        return rc;
    }
    held = std::move(nw);
    return RT_OK;
}

// out[M][N] = act(A[M][K] W^T + bias) (+ residual), float32 activations fed as hi + lo planes
int stt_gemm(rt_stt* s, const float* A, int M, const PackedW& W, const float* bias, int act, const float* residual, float* out) {
    GemmA a; a.ptr = A; a.is_f32 = 1; a.split = 1; a.M = M; a.Cin = W.K; a.taps = 1;
    GemmEpi e; e.bias = bias; e.act = act; e.residual = residual; e.out_f32 = out; e.ldc = W.N;
    return launch_gemm(s->ctx, a, W, e);
}
// M rows of x, ldx elements apart -> dense rows of out
int stt_ln(rt_stt* s, const float* x, int64_t ldx, int M, const float* w, const float* b, float* out) {
    hipLaunchKernelGGL(k_layernorm, dim3(M), dim3(256), 0, s->ctx->stream, x, ldx, s->cfg.d_model, w, b, 1e-5f, out);
    RT_HIP(s->ctx, hipGetLastError());
    return RT_OK;
}

// frames of a window that can see audio: [f hop - n_fft/2, f hop + n_fft/2) meets [0, n16); the rest are the constant of silence
int stt_frames_with_audio(const rt_stt_config& c, int64_t n16) {
    const int n_frames = (int)((int64_t)c.chunk_seconds * c.sample_rate / c.hop);     // 3000 (the last of the 3001 STFT frames is dropped)
    return n16 <= 0 ? 0 : (int)std::min<int64_t>(n_frames, (n16 + c.n_fft / 2 + c.hop - 1) / c.hop + 1);
}

// One window of the input of a call
// (key: what the sampled decode of a fallback policy keys the window's draws by - its index in its clip on the fixed-cut path, its
// start in ticks on the seek path)
struct SttSpan { int clip; const float* pcm; int64_t n; uint32_t key = 0; };

// Cuts every clip into consecutive chunk_seconds windows of the INPUT (an empty clip is one window of silence); first_only keeps a
// clip's first window alone
void stt_cut(const rt_stt_config& c, int sr, const float* const* d_pcm, const int64_t* n_samples, int n_clips, std::vector<SttSpan>& all, bool first_only = false) {
    const int64_t win = (int64_t)c.chunk_seconds * sr;              // one window, in input samples
    for (int i = 0; i < n_clips; ++i)
        for (int64_t off = 0; off == 0 || (off < n_samples[i] && !first_only); off += win)
            all.push_back({i, n_samples[i] > 0 ? d_pcm[i] + off : nullptr, std::min<int64_t>(win, n_samples[i] - off), (uint32_t)(off / win)});
}

// The front end of a group: B windows (device pointers at rate sr) -> log-mel [B][frames][n_mels] in s->grp.enc.mel, one launch per
// stage for the whole group.  The resampler's taps see all spans[b].n samples; at most one chunk of its output is kept.
int stt_features_group(rt_stt* s, const SttSpan* spans, int B, int sr) {
    rt_ctx* ctx = s->ctx;
    const rt_stt_config& c = s->cfg;
    SttEnc& w = s->grp.enc;
    const int64_t n_pad = (int64_t)c.chunk_seconds * c.sample_rate;
    const bool resample = sr != c.sample_rate;
    if (resample) RT_TRY(resampler_design(ctx, s->rs, sr, c.sample_rate));
    s->h_wins.assign(B, SttWin{});
    int64_t max16 = 0;
    int max_comp = 0;
    for (int b = 0; b < B; ++b) {
        SttWin& h = s->h_wins[b];
        h.pcm_in = spans[b].pcm;
        h.n_in = spans[b].n;
        h.n16 = std::min<int64_t>(resample ? s->rs.n_out(h.n_in) : h.n_in, n_pad);
        h.pcm16 = resample ? w.pcm16k + (size_t)b * n_pad : h.pcm_in;
        h.n_comp = stt_frames_with_audio(c, h.n16);
        max16 = std::max(max16, h.n16);
        max_comp = std::max(max_comp, h.n_comp);
    }
    RT_HIP(ctx, hipMemcpyAsync(w.d_wins, s->h_wins.data(), (size_t)B * sizeof(SttWin), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_stt_fill_i32, dim3(1), dim3(64), 0, ctx->stream, w.d_gmax, B, (int)0x80000000, 0);    // below every ordered float
    RT_HIP(ctx, hipGetLastError());
    if (resample && max16 > 0) {
        hipLaunchKernelGGL(k_resample_group, dim3((unsigned)std::min<int64_t>((max16 + 255) / 256, 4096), B), dim3(256), 0, ctx->stream, w.d_wins, w.pcm16k,
                           n_pad, s->rs.L, s->rs.M, s->rs.taps, s->rs.half, s->rs.d_h);
        RT_HIP(ctx, hipGetLastError());
    }
    const int n_frames = (int)(n_pad / c.hop), n_bins = c.n_fft / 2 + 1;
    const int64_t tot = (int64_t)n_frames * c.n_mels;
    if (max_comp > 0) {
        const size_t lds = (size_t)(3 * c.n_fft + n_bins) * sizeof(double);
        hipLaunchKernelGGL(k_logmel_frames_group, dim3(max_comp, B), dim3(256), lds, ctx->stream, w.d_wins, n_pad, c.n_fft, c.hop, n_bins, c.n_mels,
                           s->d_twc, s->d_tws, s->d_window, s->d_melT, w.mel, tot, w.d_gmax);
        RT_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_logmel_finish_group, dim3((unsigned)std::min<int64_t>((tot + 255) / 256, 2048), B), dim3(256), 0, ctx->stream, w.d_wins, w.mel, tot,
                       c.n_mels, w.d_gmax);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

// Events around the launches of one class while rt_debug_stt_align_timing is on (off: nothing is created or recorded)
struct SttAlignSpan {
    rt_stt* s; int cls; hipEvent_t a = nullptr, b = nullptr;
    SttAlignSpan(rt_stt* s_, int cls_) : s(s_), cls(cls_) {
        if (!s->al_clock) return;
        if (hipEventCreate(&a) != hipSuccess) { a = nullptr; return; }
        if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); a = b = nullptr; return; }
        (void)hipEventRecord(a, s->ctx->stream);
    }
    ~SttAlignSpan() {
        if (!a || !b) return;
        (void)hipEventRecord(b, s->ctx->stream);
        s->al_events[cls].push_back({a, b});
    }
};
// (behind the group's synchronisation)
void stt_align_clock_collect(rt_stt* s) {
    for (int c = 0; c < 3; ++c) {
        for (auto& e : s->al_events[c]) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) s->al_ms[c] += (double)ms;
            (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second);
        }
        s->al_events[c].clear();
    }
}

// one pre-LN layer over M rows of k.x (in place).  self-attention over cache `kv` (row r is written at slot[r], wpos[r] + pos_add and
// attends up to apos[r]); cross != null: the decoder's encoder-attention block between the two, over slot cross_slot[r] of *cross up
// to cross_last[r].  cap (rt_stt_align; null everywhere else, and then every launch is what it was): the layer's alignment heads get
// their cross-attention probabilities written out by a launch of their own beside the attention launch, which is left as it is
int stt_layer(rt_stt* s, const std::string& p, const SttWork& k, int M, const KvCache& kv, int layer, const int32_t* slot, const int32_t* wpos,
              const int32_t* apos, int pos_add, const KvCache* cross = nullptr, const int32_t* cross_slot = nullptr, const int32_t* cross_last = nullptr,
              const SttCapture* cap = nullptr) {
    rt_ctx* ctx = s->ctx;
    const rt_stt_config& c = s->cfg;
    const int H = c.heads, d = c.d_model / c.heads, D = c.d_model;
    float *x = k.x, *xn = k.xn, *qkv = k.qkv, *q = k.q, *ao = k.ao, *ff = k.ff;
    RT_TRY(stt_ln(s, x, D, M, SVEC(s, p + ".ln1_w"), SVEC(s, p + ".ln1_b"), xn));
    RT_TRY(stt_gemm(s, xn, M, SPW(s, p + ".wqkv"), SVEC(s, p + ".bqkv"), ACT_NONE, nullptr, qkv));
    RT_TRY(launch_qkv_post(ctx, qkv, 1, M, H, H, d, nullptr, nullptr, 0.f, nullptr, nullptr, slot, wpos, pos_add, q, kv, layer));
    RT_TRY(launch_attention(ctx, q, M, H, H, d, slot, apos, apos == wpos ? pos_add : 0, 0, kv, layer, nullptr, nullptr, 0, ao));
    RT_TRY(stt_gemm(s, ao, M, SPW(s, p + ".wo"), SVEC(s, p + ".bo"), ACT_NONE, x, x));
    if (cross) {
        RT_TRY(stt_ln(s, x, D, M, SVEC(s, p + ".lnc_w"), SVEC(s, p + ".lnc_b"), xn));
        RT_TRY(stt_gemm(s, xn, M, SPW(s, p + ".cwq"), SVEC(s, p + ".cbq"), ACT_NONE, nullptr, q));
        RT_TRY(launch_attention(ctx, q, M, H, H, d, cross_slot, cross_last, 0, 0, *cross, layer, nullptr, nullptr, 0, ao));
        if (cap && cap->per_layer[layer].n > 0) {
            SttAlignSpan span(s, 0);
            RT_TRY(launch_align_probs(ctx, q, H, d, *cross, layer, cap->rows, cap->n_rows, cap->per_layer[layer], cap->head_stride, cap->W));
        }
        RT_TRY(stt_gemm(s, ao, M, SPW(s, p + ".cwo"), SVEC(s, p + ".cbo"), ACT_NONE, x, x));
    }
    RT_TRY(stt_ln(s, x, D, M, SVEC(s, p + ".ln2_w"), SVEC(s, p + ".ln2_b"), xn));
    RT_TRY(stt_gemm(s, xn, M, SPW(s, p + ".fc1"), SVEC(s, p + ".fc1_b"), ACT_GELU, nullptr, ff));
    RT_TRY(stt_gemm(s, ff, M, SPW(s, p + ".fc2"), SVEC(s, p + ".fc2_b"), ACT_NONE, x, x));
    return RT_OK;
}

// log-mel of B windows in w.mel -> encoder states in w.out [B][n_ctx][D], and the decoders' cross-attention K/V cache.
// Every launch runs over the B windows' rows; the convolutions' taps stop at a window's ends (rows_out / rows_in).
int stt_encode(rt_stt* s, SttEnc& w, int B) {
    rt_ctx* ctx = s->ctx;
    const rt_stt_config& c = s->cfg;
    const int D = c.d_model, T2 = 2 * c.n_ctx, T = c.n_ctx;
    const SttWork& k = w.work;
    {   // conv1: k = 3, pad 1, GELU, on [T2][n_mels]
        GemmA a; a.ptr = w.mel; a.is_f32 = 1; a.split = 1; a.M = (int64_t)B * T2; a.Cin = c.n_mels; a.taps = 3; a.tap_stride = 1; a.tap_offset = -1; a.rows_out = T2; a.rows_in = T2;
        GemmEpi e; e.bias = SVEC(s, "enc.conv1_b"); e.act = ACT_GELU; e.out_f32 = w.c1; e.ldc = D;
        RT_TRY(launch_gemm(ctx, a, SPW(s, "enc.conv1"), e));
    }
    {   // conv2: k = 3, stride 2, pad 1, GELU, + positions.  Over rows [x[2t], x[2t+1]] it is the 2-tap GEMM (row t-1, row t) with the
        // weight laid out as [0 | W0 | W1 | W2]
        GemmA a; a.ptr = w.c1; a.is_f32 = 1; a.split = 1; a.M = (int64_t)B * T; a.Cin = 2 * D; a.taps = 2; a.tap_stride = 1; a.tap_offset = -1; a.rows_out = T; a.rows_in = T;
        GemmEpi e; e.bias = SVEC(s, "enc.conv2_b"); e.act = ACT_GELU; e.residual = SVEC(s, "enc.pos"); e.out_f32 = k.x; e.ldc = D;
        if (B > 1) {    // the residual is read per output row: the positions are laid under every window first, and updated in place
            hipLaunchKernelGGL(k_stt_repeat, dim3(1024), dim3(256), 0, ctx->stream, SVEC(s, "enc.pos"), (int64_t)T * D, B, k.x);
            RT_HIP(ctx, hipGetLastError());
            e.residual = k.x;
        }
        RT_TRY(launch_gemm(ctx, a, SPW(s, "enc.conv2"), e));
    }
    const int M = B * T;
    for (int i = 0; i < c.enc_layers; ++i) RT_TRY(stt_layer(s, "enc.l" + std::to_string(i), k, M, w.kv, i, w.slot, w.pos, w.last, 0));
    RT_TRY(stt_ln(s, k.x, D, M, SVEC(s, "enc.ln_w"), SVEC(s, "enc.ln_b"), w.out));
    // cross-attention K / V of every decoder layer (k_proj has no bias: its half of cbkv is zero)
    for (int i = 0; i < c.dec_layers; ++i) {
        const std::string p = "dec.l" + std::to_string(i);
        RT_TRY(stt_gemm(s, w.out, M, SPW(s, p + ".cwkv"), SVEC(s, p + ".cbkv"), ACT_NONE, nullptr, k.qkv));
        RT_TRY(launch_qkv_post(ctx, k.qkv, 1, M, 0, c.heads, D / c.heads, nullptr, nullptr, 0.f, nullptr, nullptr, w.slot, w.pos, 0, k.q, w.cross_kv, i));
    }
    return RT_OK;
}

// B x per decoder rows (tokens d.tok, row r = window r / per at position pos0 + r % per; slot / pos: its row tables into d.kv) ->
// logits of the LAST row of every window in d.logits [B][vocab].  cross_slot: the rows' slots of the cross-attention cache `cross`
int stt_decode_rows(rt_stt* s, const SttDec& d, const KvCache& cross, int B, int per, int pos0, const int32_t* slot, const int32_t* pos, const int32_t* cross_slot) {
    rt_ctx* ctx = s->ctx;
    const rt_stt_config& c = s->cfg;
    const int D = c.d_model, M = B * per;
    const SttWork& k = d.work;
    SttSlot* tok = stt_find(s, "dec.tok");
    hipLaunchKernelGGL(k_stt_embed, dim3(M), dim3(128), 0, ctx->stream, tok->tbl, SVEC(s, "dec.pos"), d.tok, pos0, per, D, k.x);
    RT_HIP(ctx, hipGetLastError());
    for (int i = 0; i < c.dec_layers; ++i) RT_TRY(stt_layer(s, "dec.l" + std::to_string(i), k, M, d.kv, i, slot, pos, pos, pos0, &cross, cross_slot, d.enc_last));
    RT_TRY(stt_ln(s, k.x + (size_t)(per - 1) * D, (int64_t)per * D, B, SVEC(s, "dec.ln_w"), SVEC(s, "dec.ln_b"), k.xn));
    RT_TRY(stt_gemm(s, k.xn, B, tok->pw, nullptr, ACT_NONE, nullptr, d.logits));
    return RT_OK;
}

// The handle's buffer set holds at least B windows: a larger one replaces it when a call needs more (stt_reserve)
int stt_group_reserve(rt_stt* s, int B) {
    if (s->grp.B >= B) return RT_OK;
    return stt_reserve(s, s->grp, [&](SttGroup& nw) { return stt_alloc_group(s, nw, B); });
}

// Greedy decode of the B encoded windows of the group: ids[b] = the first `budget` ids of window b (forced prefix in one pass, then
// one token per pass until end-of-sequence).  One device-to-host read (the rows' tokens) and one synchronisation per step for the
// whole group.  d_prefix [B][n_prefix]: every window's forced prefix (the three greedy entry points pass the handle's own, the same
// for every window).  d_first_logits: receives row 0's logits behind the prefix pass.
int stt_decode_group(rt_stt* s, int B, int budget, const int32_t* d_prefix, std::vector<std::vector<int32_t>>& ids, float* d_first_logits) {
    rt_ctx* ctx = s->ctx;
    const rt_stt_config& c = s->cfg;
    SttGroup& w = s->grp;
    const int P = c.n_prefix;
    w.dec.tok = d_prefix;
    RT_TRY(stt_decode_rows(s, w.dec, w.enc.cross_kv, B, P, 0, w.pre_slot, w.pre_pos, w.pre_slot));
    if (d_first_logits) RT_HIP(ctx, hipMemcpyAsync(d_first_logits, w.dec.logits, (size_t)c.vocab * 4, hipMemcpyDeviceToDevice, ctx->stream));
    w.dec.tok = w.d_tok;
    ids.assign(B, {});
    std::vector<char> done(B, 0);
    s->h_tok.resize(B);
    int live = B;
    for (int step = 0; step < budget; ++step) {
        hipLaunchKernelGGL(k_stt_pick, dim3(B), dim3(1024), 0, ctx->stream, w.dec.logits, c.vocab, s->d_mask, step == 0 ? 1 : 0, w.d_tok);
        RT_HIP(ctx, hipGetLastError());
        RT_HIP(ctx, hipMemcpyAsync(s->h_tok.data(), w.d_tok, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int b = 0; b < B; ++b) {
            if (done[b]) continue;
            if (s->h_tok[b] == c.eos_id) { done[b] = 1; --live; }
            else ids[b].push_back(s->h_tok[b]);
        }
        if (live <= 0) break;
        if (step + 1 < budget) RT_TRY(stt_decode_rows(s, w.dec, w.enc.cross_kv, B, 1, P + step, w.step_slot, w.step_pos, w.step_slot));
    }
    return RT_OK;
}

// Greedy transcription of n_clips clips, what rt_stt_transcribe (one clip) and rt_stt_transcribe_batch share: up to STT_GROUP
// windows go through the front end, the encoder and the greedy decode together, and a clip's ids are its windows' ids joined and
// cut at the cap.  No window is decoded past the cap (it could not contribute more ids); a window is left out only when the groups
// before it already filled its clip's cap.  d_first_logits: the first window's logits behind the forced prefix.
int stt_transcribe_greedy(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int n_clips, int sr, int32_t* h_tokens, int cap, int32_t* h_n_tokens,
                          float* d_first_logits) {
    const rt_stt_config& c = s->cfg;
    std::vector<SttSpan> all, group;
    stt_cut(c, sr, d_pcm, n_samples, n_clips, all);
    std::fill(h_n_tokens, h_n_tokens + n_clips, 0);
    RT_TRY(stt_group_reserve(s, (int)std::min<size_t>(all.size(), STT_GROUP)));
    const int budget = std::min(std::min(c.max_new_tokens, c.n_text_ctx - c.n_prefix), cap);
    std::vector<std::vector<int32_t>> ids;
    for (size_t next = 0; next < all.size();) {
        group.clear();
        for (; next < all.size() && (int)group.size() < STT_GROUP; ++next)
            if (h_n_tokens[all[next].clip] < cap) group.push_back(all[next]);
        if (group.empty()) break;
        const int B = (int)group.size();
        RT_TRY(stt_features_group(s, group.data(), B, sr));
        RT_TRY(stt_encode(s, s->grp.enc, B));
        RT_TRY(stt_decode_group(s, B, budget, s->grp.d_prefix, ids, d_first_logits));
        d_first_logits = nullptr;
        for (int b = 0; b < B; ++b) {
            const int i = group[b].clip;
            for (int32_t t : ids[b])
                if (h_n_tokens[i] < cap) h_tokens[(size_t)i * cap + h_n_tokens[i]++] = t;
        }
    }
    return RT_OK;
}

// the bookkeeping of k_stt_beam_select laid over one int32 allocation of R rows and `steps` steps (sizes in SttBeamBook's comments)
size_t stt_beam_book_words(int R, int steps) { return (size_t)11 * R + 1 + (size_t)2 * steps * R; }
SttBeamBook stt_beam_book(int32_t* mem, int R, int steps) {
    SttBeamBook b;
    int32_t* p = mem;
    auto take = [&](size_t n) { int32_t* q = p; p += n; return q; };
    b.next_tok = take(R); b.src = take(R); b.score = (float*)take(R);
    b.n_live = take(R); b.n_fin = take(R); b.done = take(R);
    b.fin_step = take(R); b.fin_beam = take(R); b.fin_score = (float*)take(R);
    b.live = take(1);
    b.bp_tok = take((size_t)steps * R); b.bp_par = take((size_t)steps * R);
    b.ts_flags = take(R); b.ts_last = take(R);
    b.R = R;
    return b;
}

// The beam path holds at least `rows` decoder rows: allocated by the first beam call, replaced when a call needs more (stt_reserve)
int stt_beam_reserve(rt_stt* s, int rows) {
    if (s->beam.rows >= rows) return RT_OK;
    return stt_reserve(s, s->beam, [&](SttBeam& nb) -> int {
        const rt_stt_config& c = s->cfg;
        const size_t r = (size_t)rows, rp = r * c.n_prefix;
        RT_TRY(stt_alloc_dec(s, nb.owned, rows, nb.dec));
        RT_TRY(stt_kv(s, nb.owned, nb.kv_next, c.dec_layers, rows, c.n_text_ctx));
        RT_TRY(stt_alloc(s, nb.owned, rp, &nb.pre_slot)); RT_TRY(stt_alloc(s, nb.owned, rp, &nb.pre_pos)); RT_TRY(stt_alloc(s, nb.owned, rp, &nb.pre_win));
        RT_TRY(stt_alloc(s, nb.owned, r, &nb.row_slot)); RT_TRY(stt_alloc(s, nb.owned, r, &nb.row_win)); RT_TRY(stt_alloc(s, nb.owned, r, &nb.row_pos));
        nb.book_n = stt_beam_book_words(rows, c.max_new_tokens);
        RT_TRY(stt_alloc(s, nb.owned, nb.book_n, &nb.book_mem));
        nb.book = stt_beam_book(nb.book_mem, rows, c.max_new_tokens);
        RT_TRY(stt_alloc(s, nb.owned, 4 * rp + 4 * r, &nb.smp));
        hipLaunchKernelGGL(k_stt_fill_i32, dim3(1), dim3(64), 0, s->ctx->stream, nb.row_pos, rows, 0, 0);
        RT_HIP(s->ctx, hipGetLastError());
        nb.rows = rows;
        return RT_OK;
    });
}

int stt_beam_reorder(rt_ctx* ctx, const KvCache& from, const KvCache& to, const int32_t* d_src, int rows, int len) {
    if (len <= 0 || rows <= 0) return RT_OK;
    SttKvPlanes p{{from.k, from.v, from.k_lo, from.v_lo}, {to.k, to.v, to.k_lo, to.v_lo}};
    hipLaunchKernelGGL(k_stt_beam_reorder, dim3(from.kv_heads, rows, from.layers), dim3(256), 0, ctx->stream, p, d_src, from.slots, from.kv_heads, from.max_pos,
                       from.head_dim, std::min(len, from.max_pos));
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

// The ranged form: row r takes positions [lo[r], hi[r]) of row src[r]; `from` and `to` may be one cache (rows that continue themselves
// are passed by).  The caller has proved 0 <= lo <= hi <= max_pos on the host; the kernel clamps all the same.
int stt_beam_reorder_range(rt_ctx* ctx, const KvCache& from, const KvCache& to, const int32_t* d_src, const int32_t* d_lo, const int32_t* d_hi, int rows) {
    if (rows <= 0) return RT_OK;
    SttKvPlanes p{{from.k, from.v, from.k_lo, from.v_lo}, {to.k, to.v, to.k_lo, to.v_lo}};
    hipLaunchKernelGGL(k_stt_beam_reorder_range, dim3(from.kv_heads, rows, from.layers), dim3(256), 0, ctx->stream, p, d_src, d_lo, d_hi, from.slots, from.kv_heads,
                       from.max_pos, from.head_dim, from.k == to.k ? 1 : 0);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

// ---------------------------------------------------------------------------------------------- conditioning on previous text (host side)
// The longest prompt a window takes, and the longest prefix that makes: <|startofprev|>, the prompt, the timestamp-mode prefix
int stt_prompt_cap(const rt_stt_config& c) { return c.n_text_ctx / 2 - 1; }
int stt_max_prefix(const rt_stt_config& c) { return 1 + stt_prompt_cap(c) + c.n_prefix - 1; }

// The prompt side holds at least `wins` windows and `rows` decoder rows (stt_reserve, as the beam path's)
int stt_prompt_reserve(rt_stt* s, int wins, int rows) {
    if (s->prm.wins >= wins && s->prm.rows >= rows) return RT_OK;
    wins = std::max(wins, s->prm.wins); rows = std::max(rows, s->prm.rows);
    return stt_reserve(s, s->prm, [&](SttPrompt& np) -> int {
        const rt_stt_config& c = s->cfg;
        const size_t cr = (size_t)wins * stt_max_prefix(c);
        RT_TRY(stt_alloc_work(s, np.owned, cr, np.work));
        RT_TRY(stt_alloc(s, np.owned, (size_t)wins * c.d_model, &np.xlast));
        RT_TRY(stt_alloc(s, np.owned, cr, &np.enc_last));
        np.tab_n = 4 * cr + 2 * (size_t)wins + 4 * (size_t)rows + 2 * (size_t)c.max_new_tokens * rows;
        RT_TRY(stt_alloc(s, np.owned, np.tab_n, &np.tab));
        hipLaunchKernelGGL(k_stt_fill_i32, dim3(64), dim3(256), 0, s->ctx->stream, np.enc_last, (int)cr, c.n_ctx - 1, 0);
        RT_HIP(s->ctx, hipGetLastError());
        np.wins = wins; np.rows = rows;
        return RT_OK;
    });
}

// Lays the tables of one decode out in s->h_prm (SttPrTab) and uploads them: nN windows of `per` decoder rows each, window k of the
// decode being window need[k] of the group (null: k itself) with the prefix tokens toks[k] (forced entries as markers).  Memory
// safety is decided here, before the decode's first launch: every prefix length, every position a pass will write and every table
// entry is checked against what was allocated; a failure launches nothing.
int stt_prompt_tables(rt_stt* s, const std::vector<std::vector<int32_t>>& toks, const int* need, int nN, int per) {
    const rt_stt_config& c = s->cfg;
    const SttPrompt& pm = s->prm;
    SttPrTab& t = s->pr_tab;
    t = SttPrTab{};
    t.nW = nN; t.rows = nN * per;
    for (int k = 0; k < nN; ++k) {
        const int P = (int)toks[k].size();
        if (P < 1 || P > stt_max_prefix(c) || P > c.n_text_ctx - 1) return rt_fail(s->ctx, RT_ERR_INVALID, "prompt: a prefix of %d tokens (1 .. %d)", P, std::min(stt_max_prefix(c), c.n_text_ctx - 1));
        t.M += P;
        t.longest = std::max(t.longest, P);
        t.steps = std::max(t.steps, std::min(c.max_new_tokens, c.n_text_ctx - P));
    }
    if (nN < 1 || nN > pm.wins || t.rows > pm.rows || t.rows > s->beam.rows || (size_t)t.M > (size_t)pm.wins * stt_max_prefix(c))
        return rt_fail(s->ctx, RT_ERR_INVALID, "prompt: %d windows of %d rows do not fit the buffers reserved for them", nN, per);
    size_t at = 0;
    auto take = [&](size_t n) { const size_t q = at; at += n; return q; };
    t.pre_slot = take(t.M); t.pre_pos = take(t.M); t.pre_win = take(t.M); t.pre_tok = take(t.M);
    t.last_row = take(nN); t.win_budget = take(nN);
    t.row_budget = take(t.rows); t.base = take(t.rows); t.zero = take(t.rows); t.fan_src = take(t.rows);
    t.step_pos = take((size_t)t.steps * t.rows); t.step_hi = take((size_t)t.steps * t.rows);
    t.total = at;
    if (t.total > pm.tab_n) return rt_fail(s->ctx, RT_ERR_INVALID, "prompt: tables of %zu entries, room for %zu", t.total, pm.tab_n);
    t.retire_win.assign(t.steps + 1, 0); t.retire_row.assign(t.steps + 1, 0);
    std::vector<int32_t>& h = s->h_prm;
    h.assign(t.total, 0);
    int row = 0;
    for (int k = 0; k < nN; ++k) {
        const int P = (int)toks[k].size(), budget = std::min(c.max_new_tokens, c.n_text_ctx - P);     // (P + budget - 1 <= n_text_ctx - 1)
        for (int i = 0; i < P; ++i, ++row) {
            h[t.pre_slot + row] = k * per; h[t.pre_pos + row] = i; h[t.pre_win + row] = need ? need[k] : k; h[t.pre_tok + row] = toks[k][i];
        }
        h[t.last_row + k] = row - 1;
        h[t.win_budget + k] = budget;
        if (budget < t.steps) t.retire_win[budget] = t.retire_row[budget] = 1;
        for (int r = k * per; r < (k + 1) * per; ++r) {
            h[t.row_budget + r] = budget; h[t.base + r] = P; h[t.fan_src + r] = k * per;
            for (int st = 0; st < t.steps; ++st) {
                h[t.step_pos + (size_t)st * t.rows + r] = std::min(P + st, P + budget - 1);
                h[t.step_hi + (size_t)st * t.rows + r] = std::min(P + st, P + budget);
            }
        }
    }
    RT_HIP(s->ctx, hipMemcpyAsync(pm.tab, h.data(), t.total * 4, hipMemcpyHostToDevice, s->ctx->stream));
    return RT_OK;
}

// M decoder rows under row tables - row r: token tok[r] at position pos[r] of slot slot[r] of `kv`, over slot cross_slot[r] of the
// cross-attention cache - through the launches stt_decode_rows issues, with the embedding reading the row's position from the
// table.  take (null: every row, n_out = M): the rows whose logits are wanted, n_out of them -> d_logits [n_out][vocab].
// (stt_decode_tab_rows: the embedding and the decoder layers of such a pass, k.x holding every row's state behind the last layer - what
//  stt_decode_tab runs in front of its tail, and what rt_stt_align runs, with the capture argument set, in front of a tail of its own)
int stt_decode_tab_rows(rt_stt* s, const SttWork& k, const KvCache& kv, const KvCache& cross, int M, const int32_t* tok, const int32_t* slot, const int32_t* pos,
                        const int32_t* cross_slot, const int32_t* enc_last, const SttCapture* cap = nullptr) {
    rt_ctx* ctx = s->ctx;
    const rt_stt_config& c = s->cfg;
    hipLaunchKernelGGL(k_stt_embed_rows, dim3(M), dim3(128), 0, ctx->stream, stt_find(s, "dec.tok")->tbl, SVEC(s, "dec.pos"), tok, pos, c.d_model, k.x);
    RT_HIP(ctx, hipGetLastError());
    for (int i = 0; i < c.dec_layers; ++i) RT_TRY(stt_layer(s, "dec.l" + std::to_string(i), k, M, kv, i, slot, pos, pos, 0, &cross, cross_slot, enc_last, cap));
    return RT_OK;
}
int stt_decode_tab(rt_stt* s, const SttWork& k, const KvCache& kv, const KvCache& cross, int M, const int32_t* tok, const int32_t* slot, const int32_t* pos,
                   const int32_t* cross_slot, const int32_t* enc_last, const int32_t* take, int n_out, float* d_logits) {
    rt_ctx* ctx = s->ctx;
    const rt_stt_config& c = s->cfg;
    const int D = c.d_model;
    SttSlot* emb = stt_find(s, "dec.tok");
    RT_TRY(stt_decode_tab_rows(s, k, kv, cross, M, tok, slot, pos, cross_slot, enc_last));
    const float* last = k.x;
    if (take) {
        hipLaunchKernelGGL(k_stt_take_rows, dim3(n_out), dim3(64), 0, ctx->stream, k.x, take, D, s->prm.xlast);
        RT_HIP(ctx, hipGetLastError());
        last = s->prm.xlast;
    }
    RT_TRY(stt_ln(s, last, D, n_out, SVEC(s, "dec.ln_w"), SVEC(s, "dec.ln_b"), k.xn));
    RT_TRY(stt_gemm(s, k.xn, n_out, emb->pw, nullptr, ACT_NONE, nullptr, d_logits));
    return RT_OK;
}

// The ragged prefix pass of the decode whose tables are up (s->pr_tab): every window's prefix rows in one pass into the cache slot of
// the window's first row of `kv`, the logits of every window's last prefix row -> d_logits [nW][vocab].  resolve: the forced entries
// are markers, filled in from s->d_win_prefix first (P entries per window of the group).
int stt_prompt_prefix_pass(rt_stt* s, const KvCache& kv, float* d_logits, bool resolve, int P) {
    const SttPrTab& t = s->pr_tab;
    int32_t* tab = s->prm.tab;
    if (resolve) {
        hipLaunchKernelGGL(k_stt_prompt_tokens, dim3((t.M + 255) / 256), dim3(256), 0, s->ctx->stream, tab + t.pre_tok, tab + t.pre_win, t.M, s->d_win_prefix, P);
        RT_HIP(s->ctx, hipGetLastError());
    }
    return stt_decode_tab(s, s->prm.work, kv, s->grp.enc.cross_kv, t.M, tab + t.pre_tok, tab + t.pre_slot, tab + t.pre_pos, tab + t.pre_win, s->prm.enc_last,
                          tab + t.last_row, t.nW, d_logits);
}
// The prefix tokens of a window under a prompt policy: <|startofprev|>, the prompt and the P forced entries (as markers), or - without
// a prompt - the forced entries alone
void stt_prompt_prefix_tokens(rt_stt* s, const std::vector<int32_t>& prompt, int P, std::vector<int32_t>& out) {
    out.clear();
    if (!prompt.empty()) { out.push_back(s->pr.sot_prev_id); out.insert(out.end(), prompt.begin(), prompt.end()); }
    for (int k = 0; k < P; ++k) out.push_back(-(1 + k));
}
// Units (windows of the beam path, rows of the sampled one) whose budget is `step` stop before that step
int stt_retire(rt_stt* s, const SttBeamBook& bk, bool by_row, int step) {
    const SttPrTab& t = s->pr_tab;
    const std::vector<char>& at = by_row ? t.retire_row : t.retire_win;
    if (step >= (int)at.size() || !at[step]) return RT_OK;
    const int n = by_row ? t.rows : t.nW;
    hipLaunchKernelGGL(k_stt_retire, dim3((n + 63) / 64), dim3(64), 0, s->ctx->stream, bk.done, bk.live, s->prm.tab + (by_row ? t.row_budget : t.win_budget), n, step);
    RT_HIP(s->ctx, hipGetLastError());
    return RT_OK;
}
// What beam search and sampled decoding share around the group's book (s->beam.book).  Before the first step: zeros, every row's next
// token end-of-sequence and its source itself, `live` units decoding (windows of the beam path, rows of the sampled one)
int stt_book_reset(rt_stt* s, int live) {
    rt_ctx* ctx = s->ctx;
    SttBeam& bm = s->beam;
    RT_HIP(ctx, hipMemsetAsync(bm.book_mem, 0, bm.book_n * 4, ctx->stream));
    hipLaunchKernelGGL(k_stt_fill_i32, dim3(1), dim3(64), 0, ctx->stream, bm.book.next_tok, bm.rows, s->cfg.eos_id, 0);
    hipLaunchKernelGGL(k_stt_fill_i32, dim3(1), dim3(64), 0, ctx->stream, bm.book.src, bm.rows, 0, 1);
    hipLaunchKernelGGL(k_stt_fill_i32, dim3(1), dim3(64), 0, ctx->stream, bm.book.live, 1, live, 0);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}
// Behind the select of `step`: under a prompt policy the units whose budget is spent retire (before the read, which then counts them
// out), then the step's one device-to-host read and one synchronisation -> the units still decoding
int stt_step_live(rt_stt* s, bool prompt, bool by_row, int step, int32_t* live) {
    if (prompt) RT_TRY(stt_retire(s, s->beam.book, by_row, step + 1));
    RT_HIP(s->ctx, hipMemcpyAsync(live, s->beam.book.live, 4, hipMemcpyDeviceToHost, s->ctx->stream));
    RT_HIP(s->ctx, hipStreamSynchronize(s->ctx->stream));
    return RT_OK;
}
// The book as the steps left it -> s->h_book, and the pointers into that copy
int stt_book_fetch(rt_stt* s, SttBeamBook* h) {
    rt_ctx* ctx = s->ctx;
    SttBeam& bm = s->beam;
    s->h_book.resize(bm.book_n);
    RT_HIP(ctx, hipMemcpyAsync(s->h_book.data(), bm.book_mem, bm.book_n * 4, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *h = stt_beam_book(s->h_book.data(), bm.rows, s->cfg.max_new_tokens);
    return RT_OK;
}

// What beam search gives for one window: the ids of the chosen hypothesis, its cumulative log-probability and the tokens it counts
// (the ids and end-of-sequence)
struct SttHyp { std::vector<int32_t> ids; float score = 0.f; int count = 1; };

// What the windows of a group take in place of the handle's prefix (stt_run_group).  Nothing set: the launches of
// rt_stt_transcribe_beam - s->grp.d_prefix for every window, nothing probed, no copy.  Otherwise a prefix per window in
// s->d_win_prefix: laid out on the host and copied in (probe false: every language is given), or written behind the probe pass by
// k_stt_lang_prefix from the group's window table in s->d_win_meta - per window its clip and the row, in this group, of its clip's
// first window (-1: an earlier group held it; s->d_clip_lang keeps what it detected).
struct SttPlan {
    const int32_t* h_req = nullptr;     // [n_clips] a clip's language, a configured id or -1 = detect; null: the handle's own
    bool probe = false;                 // the probe pass runs: a clip detects, or the windows' no-speech probabilities are wanted
    const SttTsRule* ts = nullptr;      // timestamp mode: the prefix without its last entry (<|notimestamps|>), the rule at every step
    int32_t win_first[STT_GROUP] = {};  // the window table's second column, set per group (the first, a window's clip, is in its span)
    // a fallback policy is set (rt_stt_set_fallback): the group's windows go through stt_fallback_group, which leaves here, per window
    // of the group, what rt_stt_fallback_report returns
    std::vector<SttFbWin>* fallback = nullptr;
    // a prompt policy is set (rt_stt_set_prompt; timestamp mode only): per window of the group the prompt ids it decodes behind (empty:
    // none).  The group then runs the ragged prefix pass and per-window budgets (stt_prompt_tables), whatever the prompts' lengths
    const std::vector<int32_t>* prompt = nullptr;
    bool per_window() const { return h_req || probe || ts; }
    int n_prefix(const rt_stt_config& c) const { return ts ? c.n_prefix - 1 : c.n_prefix; }
};

// k_stt_probe over nW rows of logits -> s->d_probe rows 0 .. 2
int stt_probe(rt_stt* s, const float* d_logits, int64_t row_stride, int nW) {
    int32_t* p = s->d_probe;
    hipLaunchKernelGGL(k_stt_probe, dim3(nW), dim3(1024), 0, s->ctx->stream, d_logits, row_stride, s->cfg.vocab, s->d_lang_ids, (int)s->lang_ids.size(),
                       s->no_speech_id, p, (float*)(p + STT_GROUP), (float*)(p + 2 * STT_GROUP));
    RT_HIP(s->ctx, hipGetLastError());
    return RT_OK;
}
// The probe pass over the nW encoded windows of the group on decoder side d: row w is start-of-transcript alone at position 0 of
// cache slot slot[w] (pos: zeros), over window w's encoder states, then k_stt_probe on its logits.  The greedy side
// (rt_stt_detect_language) and the beam side run the same kernels at the same shapes: a window's three results are the same bits.
int stt_probe_pass(rt_stt* s, SttDec& d, const int32_t* slot, const int32_t* pos, int nW) {
    d.tok = s->d_sot;
    RT_TRY(stt_decode_rows(s, d, s->grp.enc.cross_kv, nW, 1, 0, slot, pos, slot));
    return stt_probe(s, d.logits, s->cfg.vocab, nW);
}
// k_stt_lang_prefix over the group's window table (s->d_win_meta): the first P entries of every window's prefix into
// s->d_win_prefix, and row 3 of s->d_probe
int stt_lang_prefix(rt_stt* s, int nW, int P) {
    rt_ctx* ctx = s->ctx;
    hipLaunchKernelGGL(k_stt_lang_prefix, dim3(1), dim3(64), 0, ctx->stream, nW, P, s->grp.d_prefix, s->d_win_meta, s->d_win_meta + STT_GROUP,
                       s->d_clip_lang, s->d_probe, s->d_win_prefix, s->d_probe + 3 * STT_GROUP);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}
// The probe of a group on the beam path's decoder side, what stt_decode_beam_group and - under a fallback policy without a beam decode -
// stt_run_group share: the probe pass on cache slot w of window w (s->beam.row_slot holds the identity), then the windows' prefixes
// and the ids they took on the device
int stt_probe_group(rt_stt* s, int nW, int P) {
    SttBeam& bm = s->beam;
    RT_TRY(stt_probe_pass(s, bm.dec, bm.row_slot, bm.row_pos, nW));
    return stt_lang_prefix(s, nW, P);
}
// One step of beam search over nW windows: k_stt_beam_select, the timestamp instantiation when a rule is given
int stt_beam_select(rt_stt* s, const float* d_logits, int row_stride, int nW, int first_step, int B, int step, const SttBeamBook& bk, const SttTsRule* ts) {
    const rt_stt_config& c = s->cfg;
    auto* select = ts ? k_stt_beam_select<true> : k_stt_beam_select<false>;
    hipLaunchKernelGGL(select, dim3(nW), dim3(1024), 0, s->ctx->stream, d_logits, c.vocab, row_stride, s->d_mask, first_step, c.eos_id, B, step, bk,
                       ts ? *ts : SttTsRule{});
    RT_HIP(s->ctx, hipGetLastError());
    return RT_OK;
}

// Beam search (width B) over the nW encoded windows of the group, rows = nW B.  The prefix pass runs one row per window into the
// cache slot of the window's first beam row; the reorder kernel then fans it out to the window's rows, and after every later
// step gives row r the cache of the row it continues.  One device-to-host read and one synchronisation per step, as the greedy
// group; the bookkeeping comes back once, and the host follows the back-pointers of the finished entries.
// plan: the prefix every window takes (SttPlan) and whether the probe pass runs to decide it; in timestamp mode every step applies
// the timestamp rule (k_stt_beam_select<true>), and the ids that come back hold timestamp ids.
int stt_decode_beam_group(rt_stt* s, int nW, int B, std::vector<SttHyp>& out, const SttPlan& plan) {
    rt_ctx* ctx = s->ctx;
    const rt_stt_config& c = s->cfg;
    SttBeam& bm = s->beam;
    const int P = plan.n_prefix(c), rows = nW * B, R = bm.rows;
    const SttBeamBook& bk = bm.book;
    const KvCache& cross = s->grp.enc.cross_kv;
    RT_TRY(stt_book_reset(s, nW));
    hipLaunchKernelGGL(k_stt_fill_i32, dim3(1), dim3(64), 0, ctx->stream, bk.n_live, nW, 1, 0);
    hipLaunchKernelGGL(k_stt_fill_beam_rows, dim3(1), dim3(256), 0, ctx->stream, bm.pre_slot, bm.pre_pos, bm.pre_win, nW * P, P, B, bm.row_slot, bm.row_win, rows);
    RT_HIP(ctx, hipGetLastError());
    bm.dec.tok = s->grp.d_prefix;                // (the forced prefix of every window: the group keeps it)
    if (plan.per_window()) {
        // the probe pass on cache slot w of window w (the prefix pass and the reorder behind it overwrite what it leaves in the
        // cache), then the windows' prefixes on the device.  Every language given and no no-speech probability wanted: no launch is
        // added to those of rt_stt_transcribe_beam
        if (plan.probe) RT_TRY(stt_probe_group(s, nW, P));
        bm.dec.tok = s->d_win_prefix;        // (without a probe every language is given: stt_run_group has copied the prefixes in)
    }
    // under a prompt policy (stt_run_group has laid the tables out): the ragged prefix pass, then the prefix - which never diverges
    // between a window's beams - into every row's slot of BOTH caches, so that the gather between steps moves generated positions only
    const SttPrTab* pt = plan.prompt ? &s->pr_tab : nullptr;
    const int32_t* tab = s->prm.tab;
    if (pt) {
        RT_TRY(stt_prompt_prefix_pass(s, bm.dec.kv, bm.dec.logits, true, P));
        RT_TRY(stt_beam_reorder_range(ctx, bm.dec.kv, bm.dec.kv, tab + pt->fan_src, tab + pt->zero, tab + pt->base, rows));
        RT_TRY(stt_beam_reorder_range(ctx, bm.dec.kv, bm.kv_next, tab + pt->fan_src, tab + pt->zero, tab + pt->base, rows));
    } else {
        RT_TRY(stt_decode_rows(s, bm.dec, cross, nW, P, 0, bm.pre_slot, bm.pre_pos, bm.pre_win));
    }
    const int budget = pt ? pt->steps : std::min(c.max_new_tokens, c.n_text_ctx - P);
    int steps = 0;
    for (int step = 0; step < budget; ++step) {
        RT_TRY(stt_beam_select(s, bm.dec.logits, step == 0 ? 1 : B, nW, step == 0 ? 1 : 0, B, step, bk, plan.ts));
        steps = step + 1;
        int32_t live = 0;
        RT_TRY(stt_step_live(s, pt != nullptr, false, step, &live));
        if (live <= 0 || step + 1 >= budget) break;
        if (pt) {
            if (!g_stt_gather_ranged) {         // (the A/B of the ranged form: what the gather costs when it moves the prefix at every step)
                // (a short-prefix window sets the step count and a long-prefix one the length: cut at the cache's end)
                RT_TRY(stt_beam_reorder(ctx, bm.dec.kv, bm.kv_next, bk.src, rows, std::min(pt->longest + step, c.n_text_ctx)));
                std::swap(bm.dec.kv, bm.kv_next);
            } else if (step > 0) {              // (behind the first step nothing is generated yet, and both caches hold the prefix)
                RT_TRY(stt_beam_reorder_range(ctx, bm.dec.kv, bm.kv_next, bk.src, tab + pt->base, tab + pt->step_hi + (size_t)step * rows, rows));
                std::swap(bm.dec.kv, bm.kv_next);
            }
            RT_TRY(stt_decode_tab(s, bm.dec.work, bm.dec.kv, cross, rows, bk.next_tok, bm.row_slot, tab + pt->step_pos + (size_t)step * rows, bm.row_win,
                                  bm.dec.enc_last, nullptr, rows, bm.dec.logits));
            continue;
        }
        RT_TRY(stt_beam_reorder(ctx, bm.dec.kv, bm.kv_next, bk.src, rows, P + step));
        std::swap(bm.dec.kv, bm.kv_next);
        bm.dec.tok = bk.next_tok;
        RT_TRY(stt_decode_rows(s, bm.dec, cross, rows, 1, P + step, bm.row_slot, bm.row_pos, bm.row_win));
    }
    SttBeamBook h;
    RT_TRY(stt_book_fetch(s, &h));
    out.assign(nW, SttHyp{});
    // the tokens of beam `b` as it stood after step t: follow the back-pointers to step 0
    auto history = [&](int w, int t, int b, std::vector<int32_t>& ids) {
        ids.assign(t + 1, 0);
        for (int u = t; u >= 0; --u) {
            const size_t at = (size_t)u * R + (size_t)w * B + b;
            ids[u] = h.bp_tok[at];
            b = h.bp_par[at];
        }
    };
    for (int w = 0; w < nW; ++w) {
        // the finished list, then - if it has room left - the live beams in order; the largest score / (tokens + 1) wins, the earlier
        // entry on a tie
        bool have = false;
        double best = 0.0;
        int n_f = std::min(h.n_fin[w], B);
        auto offer = [&](int t_last, int b, float score) {
            const int count = t_last + 2;                   // t_last + 1 ids and end-of-sequence
            const double norm = (double)score / (double)count;
            if (have && !(norm > best)) return;
            have = true; best = norm;
            out[w].score = score; out[w].count = count;
            if (t_last >= 0) history(w, t_last, b, out[w].ids); else out[w].ids.clear();
        };
        for (int k = 0; k < n_f; ++k) offer(h.fin_step[w * B + k] - 1, h.fin_beam[w * B + k], h.fin_score[w * B + k]);
        // (a window that stopped at a budget of its own offers its beams as they stood at its last step)
        const int last = (pt ? std::min(steps, s->h_prm[pt->win_budget + w]) : steps) - 1;
        for (int i = 0; i < std::min(h.n_live[w], B) && n_f < B; ++i, ++n_f) offer(last, i, h.score[w * B + i]);
    }
    return RT_OK;
}

// What a group reports per window beside its hypothesis: the language its prefix took, that language's probability - the probe's
// for the window where the clip asked for detection (the clip's own on its first window), 1 where it was given: a forced language
// (or the handle's own) counts as certain, as in the reference's transcribers - and the no-speech probability (NaN without a probe)
struct SttWinInfo { int32_t lang; float lang_prob, no_speech; };

// One sampled step over `rows` rows: k_stt_sample_select, the timestamp instantiation when a rule is given
int stt_sample_select(rt_stt* s, const float* d_logits, int row_stride, int rows, int first_step, int S, int step, const SttBeamBook& bk, const SttTsRule* ts,
                      const SttSampleRule& sr, float* d_val) {
    const rt_stt_config& c = s->cfg;
    auto* select = ts ? k_stt_sample_select<true> : k_stt_sample_select<false>;
    hipLaunchKernelGGL(select, dim3(rows), dim3(1024), 0, s->ctx->stream, d_logits, c.vocab, row_stride, s->d_mask, first_step, c.eos_id, S, step, bk,
                       ts ? *ts : SttTsRule{}, sr, d_val);
    RT_HIP(s->ctx, hipGetLastError());
    return RT_OK;
}

// Sampled decoding at temperature T (> 0; index t_index of the policy) of the windows `need` of the encoded group, S independent rows
// each ("temperature fallback"): rows = need x S over the encoder states the group holds - nothing of the front
// end or the encoder runs.  The prefix pass runs one row per window into the cache slot of the window's first row and the reorder
// kernel fans it out once; after that every row continues itself and nothing is reordered.  One device-to-host read and one
// synchronisation per step.  out[k]: the row of window need[k] with the largest score / (ids + 1), the lower sample index on a tie.
int stt_decode_sample_group(rt_stt* s, const SttSpan* spans, const std::vector<int>& need, const std::vector<SttWinInfo>& info, int S, float T, int t_index,
                            const SttPlan& plan, std::vector<SttHyp>& out) {
    rt_ctx* ctx = s->ctx;
    const rt_stt_config& c = s->cfg;
    SttBeam& bm = s->beam;
    const int nN = (int)need.size(), P = plan.n_prefix(c), rows = nN * S, R = bm.rows;
    const size_t rp = (size_t)R * c.n_prefix;
    const SttBeamBook& bk = bm.book;
    const KvCache& cross = s->grp.enc.cross_kv;
    // the tables of this attempt, laid out as SttBeam::smp says
    std::vector<int32_t>& h = s->h_smp;
    h.assign(4 * rp + 4 * (size_t)R, 0);
    auto part = [&](int32_t* base, int k) { return k < 4 ? base + k * rp : base + 4 * rp + (size_t)(k - 4) * R; };
    for (int k = 0; k < nN; ++k)
        for (int i = 0; i < P; ++i) {
            const size_t at = (size_t)k * P + i;
            part(h.data(), 0)[at] = k * S; part(h.data(), 1)[at] = i; part(h.data(), 2)[at] = need[k];
            part(h.data(), 3)[at] = (i == 1 && P > 1) ? info[need[k]].lang : c.prefix[i];
        }
    for (int r = 0; r < rows; ++r) {
        part(h.data(), 4)[r] = r; part(h.data(), 5)[r] = need[r / S];
        part(h.data(), 6)[r] = (int32_t)spans[need[r / S]].key; part(h.data(), 7)[r] = r % S;
    }
    RT_HIP(ctx, hipMemcpyAsync(bm.smp, h.data(), h.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    RT_TRY(stt_book_reset(s, rows));
    // under a prompt policy every attempt of a window decodes behind the prefix its beam attempt had: the same prompt, the same tables
    // but for the rows per window
    const SttPrTab* pt = nullptr;
    const int32_t* tab = s->prm.tab;
    if (plan.prompt) {
        std::vector<std::vector<int32_t>> toks(nN);
        for (int k = 0; k < nN; ++k) stt_prompt_prefix_tokens(s, plan.prompt[need[k]], P, toks[k]);
        RT_TRY(stt_prompt_tables(s, toks, need.data(), nN, S));
        pt = &s->pr_tab;
        RT_TRY(stt_prompt_prefix_pass(s, bm.dec.kv, bm.dec.logits, true, P));
    } else {
        bm.dec.tok = part(bm.smp, 3);
        RT_TRY(stt_decode_rows(s, bm.dec, cross, nN, P, 0, part(bm.smp, 0), part(bm.smp, 1), part(bm.smp, 2)));
    }
    const SttSampleRule sr{T, (unsigned)(s->fb.seed & 0xffffffffu), (unsigned)(s->fb.seed >> 32), (unsigned)t_index, part(bm.smp, 6), part(bm.smp, 7)};
    const int budget = pt ? pt->steps : std::min(c.max_new_tokens, c.n_text_ctx - P);
    int steps = 0;
    for (int step = 0; step < budget; ++step) {
        RT_TRY(stt_sample_select(s, bm.dec.logits, step == 0 ? 1 : S, rows, step == 0 ? 1 : 0, S, step, bk, plan.ts, sr, nullptr));
        steps = step + 1;
        int32_t live = 0;
        RT_TRY(stt_step_live(s, pt != nullptr, true, step, &live));
        if (live <= 0 || step + 1 >= budget) break;
        if (step == 0 && S > 1) {                   // the window's first row holds the prefix: every row of the window takes it
            if (pt) RT_TRY(stt_beam_reorder_range(ctx, bm.dec.kv, bm.kv_next, tab + pt->fan_src, tab + pt->zero, tab + pt->base, rows));
            else RT_TRY(stt_beam_reorder(ctx, bm.dec.kv, bm.kv_next, bk.src, rows, P));
            std::swap(bm.dec.kv, bm.kv_next);
        }
        if (pt) {
            RT_TRY(stt_decode_tab(s, bm.dec.work, bm.dec.kv, cross, rows, bk.next_tok, part(bm.smp, 4), tab + pt->step_pos + (size_t)step * rows, part(bm.smp, 5),
                                  bm.dec.enc_last, nullptr, rows, bm.dec.logits));
            continue;
        }
        bm.dec.tok = bk.next_tok;
        RT_TRY(stt_decode_rows(s, bm.dec, cross, rows, 1, P + step, part(bm.smp, 4), bm.row_pos, part(bm.smp, 5)));
    }
    SttBeamBook hb;
    RT_TRY(stt_book_fetch(s, &hb));
    out.assign(nN, SttHyp{});
    std::vector<int32_t> ids;
    for (int k = 0; k < nN; ++k) {
        double best = 0.0;
        for (int j = 0; j < S; ++j) {
            const int r = k * S + j;
            ids.clear();
            const int n_steps = pt ? std::min(steps, s->h_prm[pt->row_budget + r]) : steps;      // (a row that stopped at a budget of its own)
            for (int u = 0; u < n_steps; ++u) {
                const int32_t t = hb.bp_tok[(size_t)u * R + r];
                if (t == c.eos_id) break;
                ids.push_back(t);
            }
            const int count = (int)ids.size() + 1;
            const double norm = (double)hb.score[r] / (double)count;
            if (j > 0 && !(norm > best)) continue;
            best = norm;
            out[k].ids = ids; out[k].score = hb.score[r]; out[k].count = count;
        }
    }
    return RT_OK;
}

// The per-call side of a plan with a probe: s->d_clip_lang holds every clip's request, and the probe's results have a host copy
int stt_plan_begin(rt_stt* s, const SttPlan& plan, int n_clips) {
    rt_ctx* ctx = s->ctx;
    if (!plan.probe) return RT_OK;
    if (s->clip_lang_cap < n_clips) {
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const int cap = std::max(n_clips, 2 * s->clip_lang_cap);
        RT_TRY(stt_alloc(s, s->owned, (size_t)cap, &s->d_clip_lang));          // (the smaller one stays owned until rt_stt_destroy)
        s->clip_lang_cap = cap;
    }
    // without a request every clip keeps the handle's own language
    std::vector<int32_t> req(n_clips, s->cfg.prefix[1]);
    if (plan.h_req) req.assign(plan.h_req, plan.h_req + n_clips);
    RT_HIP(ctx, hipMemcpy(s->d_clip_lang, req.data(), (size_t)n_clips * 4, hipMemcpyHostToDevice));
    s->h_probe.resize(4 * STT_GROUP);
    return RT_OK;
}

// The fallback loop over one decoded group ("temperature fallback"; faster-whisper's generate_with_fallback).
// hyps: the beam decode of every window when the first temperature is 0.  Per temperature the windows that still need an attempt are
// decoded (temperature 0: already there), and the rule is evaluated on the host: the compression ratio of the attempt's text ids (the
// caller's callback; an attempt without text ids has ratio 0 and the callback is not asked) against its threshold, the average
// log-probability against its own, and the silence exemption.  The number of attempts is bounded by n_temperatures.  On return
// hyps[w] is the chosen attempt of window w.
int stt_fallback_group(rt_stt* s, const SttSpan* spans, int nW, const SttPlan& plan, std::vector<SttHyp>& hyps, const std::vector<SttWinInfo>& info,
                       std::vector<SttFbWin>& report) {
    const rt_stt_fallback& f = s->fb;
    struct Attempt { SttHyp hyp; float T, ratio, avg; bool ratio_ok; };
    const bool cr_set = f.compression_ratio_threshold == f.compression_ratio_threshold, lp_set = f.logprob_threshold == f.logprob_threshold;
    const bool ns_set = f.no_speech_threshold == f.no_speech_threshold;
    std::vector<std::vector<Attempt>> tried(nW);
    std::vector<int> chosen(nW, -1), need(nW), next;
    for (int w = 0; w < nW; ++w) need[w] = w;
    std::vector<SttHyp> got;
    std::vector<int32_t> text;
    for (int t = 0; t < f.n_temperatures && !need.empty(); ++t) {
        const float T = f.temperatures[t];
        if (T > 0.f) RT_TRY(stt_decode_sample_group(s, spans, need, info, f.best_of, T, t, plan, got));
        else got = hyps;                                    // (t == 0, every window: the beam decode the caller ran)
        next.clear();
        for (size_t k = 0; k < need.size(); ++k) {
            const int w = need[k];
            Attempt a{std::move(got[k]), T, NAN, 0.f, true};
            a.avg = a.hyp.score / (float)a.hyp.count;
            if (f.ratio) {
                text.clear();
                for (int32_t id : a.hyp.ids)
                    if (!plan.ts || id < plan.ts->t0) text.push_back(id);
                a.ratio = text.empty() ? 0.f : f.ratio(text.data(), (int32_t)text.size(), f.ratio_user);
                if (!text.empty() && !(a.ratio > 0.f))
                    return rt_fail(s->ctx, RT_ERR_INVALID, "fallback: the ratio callback returned %g for %zu ids (a compression ratio is above 0)", (double)a.ratio, text.size());
                a.ratio_ok = !(cr_set && a.ratio > f.compression_ratio_threshold);
            }
            bool needs = !a.ratio_ok || (lp_set && a.avg < f.logprob_threshold);
            if (ns_set && lp_set && info[w].no_speech > f.no_speech_threshold && a.avg < f.logprob_threshold) needs = false;      // silence: the caller's rule
            tried[w].push_back(std::move(a));
            if (needs) next.push_back(w); else chosen[w] = (int)tried[w].size() - 1;
        }
        need.swap(next);
    }
    // every temperature failed: the largest average among the attempts within the compression threshold, among all when none is
    for (int w : need) {
        bool any_ok = false;
        for (const Attempt& a : tried[w]) any_ok = any_ok || a.ratio_ok;
        for (int k = 0; k < (int)tried[w].size(); ++k) {
            if (any_ok && !tried[w][k].ratio_ok) continue;
            if (chosen[w] < 0 || tried[w][k].avg > tried[w][chosen[w]].avg) chosen[w] = k;
        }
    }
    report.assign(nW, SttFbWin{});
    hyps.resize(nW);
    for (int w = 0; w < nW; ++w) {
        Attempt& a = tried[w][chosen[w]];
        report[w].attempts = (int32_t)tried[w].size(); report[w].temperature = a.T; report[w].ratio = a.ratio;
        hyps[w] = std::move(a.hyp);
    }
    return RT_OK;
}

// One group through the whole path, what rt_stt_transcribe_beam, rt_stt_transcribe_ex and rt_stt_transcribe_seek share: nW windows
// at rate sr -> front end, encoder, beam search of width B under the plan.  The group's uploads come first, while the stream is
// idle: a copy from pageable memory in the middle of the group would make the host wait for the encoder.
int stt_run_group(rt_stt* s, const SttSpan* spans, int nW, int sr, int B, const SttPlan& plan, std::vector<SttHyp>& hyps, std::vector<SttWinInfo>& info) {
    rt_ctx* ctx = s->ctx;
    const rt_stt_config& c = s->cfg;
    const int P = plan.n_prefix(c);
    if (plan.per_window()) {
        s->h_meta.assign((size_t)STT_GROUP * std::max(c.n_prefix, 2), -1);      // (alive until the group's synchronisation)
        if (plan.probe) {
            for (int b = 0; b < nW; ++b) { s->h_meta[b] = spans[b].clip; s->h_meta[STT_GROUP + b] = plan.win_first[b]; }
            RT_HIP(ctx, hipMemcpyAsync(s->d_win_meta, s->h_meta.data(), 2 * STT_GROUP * 4, hipMemcpyHostToDevice, ctx->stream));
        } else {        // every language is given: laid out here and copied in, which adds no launch to those of rt_stt_transcribe_beam
            for (int b = 0; b < nW; ++b)
                for (int k = 0; k < P; ++k) s->h_meta[(size_t)b * P + k] = (k == 1 && plan.h_req) ? plan.h_req[spans[b].clip] : c.prefix[k];
            RT_HIP(ctx, hipMemcpyAsync(s->d_win_prefix, s->h_meta.data(), (size_t)nW * P * 4, hipMemcpyHostToDevice, ctx->stream));
        }
    }
    // a policy whose first temperature is above 0 has no beam decode: the probe alone (stt_probe_group), behind the row tables it reads
    const bool sampled_first = plan.fallback && s->fb.temperatures[0] > 0.f;
    if (plan.prompt && !sampled_first) {       // the tables of the beam decode under a prompt policy, with the other uploads
        std::vector<std::vector<int32_t>> toks(nW);
        for (int b = 0; b < nW; ++b) stt_prompt_prefix_tokens(s, plan.prompt[b], P, toks[b]);
        RT_TRY(stt_prompt_tables(s, toks, nullptr, nW, B));
    }
    RT_TRY(stt_features_group(s, spans, nW, sr));
    RT_TRY(stt_encode(s, s->grp.enc, nW));
    if (!sampled_first) RT_TRY(stt_decode_beam_group(s, nW, B, hyps, plan));
    else if (plan.probe) {
        SttBeam& bm = s->beam;
        hipLaunchKernelGGL(k_stt_fill_beam_rows, dim3(1), dim3(256), 0, ctx->stream, bm.pre_slot, bm.pre_pos, bm.pre_win, nW * P, P, 1, bm.row_slot, bm.row_win, nW);
        RT_HIP(ctx, hipGetLastError());
        RT_TRY(stt_probe_group(s, nW, P));
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (plan.probe) RT_HIP(ctx, hipMemcpy(s->h_probe.data(), s->d_probe, 4 * STT_GROUP * 4, hipMemcpyDeviceToHost));     // (behind the group's last synchronisation)
    const float* pf = (const float*)s->h_probe.data();
    info.resize(nW);
    for (int b = 0; b < nW; ++b) {
        const int i = spans[b].clip;
        const bool detected = plan.h_req && plan.h_req[i] < 0;
        info[b].lang = plan.probe ? s->h_probe[3 * STT_GROUP + b] : plan.h_req ? plan.h_req[i] : c.prefix[P > 1 ? 1 : 0];
        info[b].lang_prob = detected ? pf[STT_GROUP + b] : 1.0f;
        info[b].no_speech = plan.probe ? pf[2 * STT_GROUP + b] : NAN;
    }
    if (plan.fallback) RT_TRY(stt_fallback_group(s, spans, nW, plan, hyps, info, *plan.fallback));
    return RT_OK;
}

// What rt_stt_transcribe_ex asks for (h_req, probe: as SttPlan's) and receives beyond ids and scores (host pointers, null: not
// asked for)
struct SttReport {
    const int32_t* h_req = nullptr;
    bool probe = false;
    int32_t* h_lang = nullptr;
    float* h_lang_prob = nullptr;
    int32_t *win_clip = nullptr, *win_n_ids = nullptr;
    float *win_logprob = nullptr, *win_no_speech = nullptr;
};

// Beam-search transcription of the windows `all` of n_clips clips, what rt_stt_transcribe_beam (rep == null: the handle's prefix for
// every window, nothing probed) and rt_stt_transcribe_ex share: floor(STT_GROUP / beam_size) windows make a group.
int stt_transcribe_beam(rt_stt* s, const std::vector<SttSpan>& all, int n_clips, int sr, int beam_size, int32_t* h_tokens, int max_tokens, int32_t* h_n_tokens,
                        float* h_scores, const SttReport* rep) {
    std::fill(h_n_tokens, h_n_tokens + n_clips, 0);
    // under a fallback policy (rt_stt_transcribe_ex only) a window takes max(beam_size, best_of) decoder rows
    const bool fallback = rep && s->fb_set;
    const int per_window = fallback ? std::max(beam_size, s->fb.best_of) : beam_size;
    const size_t per_group = (size_t)(STT_GROUP / per_window);
    const int most = (int)std::min(all.size(), per_group);
    RT_TRY(stt_group_reserve(s, most));
    RT_TRY(stt_beam_reserve(s, most * per_window));
    SttPlan plan;
    std::vector<SttFbWin> fb_group;
    if (rep) { plan.h_req = rep->h_req; plan.probe = rep->probe; }
    if (fallback) { plan.fallback = &fb_group; s->fb_report.clear(); }
    RT_TRY(stt_plan_begin(s, plan, n_clips));
    std::vector<int32_t> first_at(n_clips, -1);      // a clip's first window, among `all`
    std::vector<double> sum(n_clips, 0.0);
    std::vector<int64_t> count(n_clips, 0);
    std::vector<SttHyp> hyps;
    std::vector<SttWinInfo> info;
    for (size_t next = 0; next < all.size(); next += per_group) {
        const int nW = (int)std::min(per_group, all.size() - next);
        for (int b = 0; b < nW; ++b) {
            const int i = all[next + b].clip;
            if (next + b == 0 || all[next + b - 1].clip != i) first_at[i] = (int32_t)(next + b);
            plan.win_first[b] = first_at[i] >= (int32_t)next ? first_at[i] - (int32_t)next : -1;
        }
        RT_TRY(stt_run_group(s, all.data() + next, nW, sr, beam_size, plan, hyps, info));
        if (fallback) s->fb_report.insert(s->fb_report.end(), fb_group.begin(), fb_group.end());
        for (int b = 0; b < nW; ++b) {
            const int i = all[next + b].clip;
            for (int32_t t : hyps[b].ids)
                if (h_n_tokens[i] < max_tokens) h_tokens[(size_t)i * max_tokens + h_n_tokens[i]++] = t;
            sum[i] += (double)hyps[b].score;
            count[i] += hyps[b].count;
            if (!rep) continue;
            const size_t at = next + b;
            if (rep->win_clip) rep->win_clip[at] = i;
            if (rep->win_n_ids) rep->win_n_ids[at] = (int32_t)hyps[b].ids.size();
            if (rep->win_logprob) rep->win_logprob[at] = hyps[b].score;
            if (rep->win_no_speech) rep->win_no_speech[at] = info[b].no_speech;
            if (first_at[i] != (int32_t)at) continue;                   // the clip's first window: its language
            if (rep->h_lang) rep->h_lang[i] = info[b].lang;
            if (rep->h_lang_prob) rep->h_lang_prob[i] = info[b].lang_prob;
        }
    }
    if (h_scores)
        for (int i = 0; i < n_clips; ++i) h_scores[i] = (float)(sum[i] / (double)std::max<int64_t>(count[i], 1));
    return RT_OK;
}

// ---------------------------------------------------------------------------------------------- timestamps and seek (rt_stt_transcribe_seek)
// A closed segment of one window: start and end in ticks of the window, and its text ids (timestamps stripped)
// (raw: every id of the slice, its timestamps included - what the clip's history gains under a prompt policy)
struct SttSeg { int start = 0, end = 0; std::vector<int32_t> ids, raw; };

// The seek rule ("timestamps and seek") on one window's hypothesis `seq` (end-of-sequence stripped, timestamp
// ids are those >= t0): consecutive timestamp pairs close segments; with a single trailing timestamp the window is consumed whole;
// otherwise the tokens behind the last closed pair are discarded and the next window starts at that pair's timestamp; without any
// pair the window is one segment, consumed whole.  own: the ticks the window's own samples span; whole: a whole window in ticks.
// Returns the advance in ticks.
int stt_seek_rule(const std::vector<int32_t>& seq, int t0, int own, int whole, std::vector<SttSeg>& segs) {
    const int n = (int)seq.size();
    auto is_ts = [&](int k) { return seq[k] >= t0; };
    auto close = [&](int a, int b, int start, int end) {
        SttSeg g;
        g.start = start; g.end = end;
        g.raw.assign(seq.begin() + a, seq.begin() + b);
        for (int k = a; k < b; ++k)
            if (!is_ts(k)) g.ids.push_back(seq[k]);
        segs.push_back(std::move(g));
    };
    std::vector<int> cuts;
    for (int k = 0; k + 1 < n; ++k)
        if (is_ts(k) && is_ts(k + 1)) cuts.push_back(k + 1);
    const bool single = n >= 2 && !is_ts(n - 2) && is_ts(n - 1);
    if (!cuts.empty()) {
        if (single) cuts.push_back(n); else cuts.back() += 1;      // (the last slice keeps both timestamps of its pair)
        int last = 0;
        for (size_t i = 0; i < cuts.size(); ++i) {
            const int cur = cuts[i];
            const bool tail = i + 1 == cuts.size() && !single;
            close(last, cur, seq[last] - t0, seq[cur - (tail ? 2 : 1)] - t0);
            last = cur;
        }
        return single ? whole : seq[last - 2] - t0;
    }
    int end = own;
    for (int k = n - 1; k >= 0; --k)
        if (is_ts(k)) { if (seq[k] != t0) end = seq[k] - t0; break; }
    close(0, n, 0, end);
    return whole;
}

// What one decoded window of a seek call leaves behind
struct SttSeekWin { int clip; int64_t off; int n_ids; float logprob, no_speech; int advance; int prompt_len = 0, reset = 0; };
struct SttSeekSeg { int clip; int64_t start_tick, end_tick; int n_ids; };
struct SttSeekResult {
    std::vector<std::vector<int32_t>> ids;               // per clip: the text ids of its segments, joined
    std::vector<std::vector<SttSeekSeg>> segs;           // per clip, in order
    std::vector<std::vector<SttSeekWin>> wins;           // per clip, in order
    std::vector<std::vector<SttFbWin>> fb;               // per clip, a line per window under a fallback policy
    std::vector<float> score, lang_prob;
    std::vector<int32_t> lang;
};

// The seek loop: a round holds one window per unfinished clip at the clip's current offset (in input samples, a multiple of the
// tick); rounds go through stt_run_group in groups of floor(STT_GROUP / beam_size) windows as stt_transcribe_beam's windows do (the
// probe, if any, in front of the decode), and the host applies the silence rule and the seek rule to what a group decoded.  Every round moves
// every unfinished clip on by at least one tick, so max_rounds - computed before the first launch - bounds the loop.
int stt_transcribe_seek(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int n_clips, int sr, const rt_stt_seek_opts& o, bool probe,
                        SttSeekResult& res) {
    const rt_stt_config& c = s->cfg;
    const int beam_size = o.beam_size;
    const int64_t tick = (int64_t)(0.02 * (double)sr), win = (int64_t)c.chunk_seconds * sr;
    const int whole = s->ts_count - 1;
    const SttTsRule rule{s->ts_begin, s->ts_count, o.max_initial_timestamp_index};
    SttPlan plan;
    plan.h_req = o.h_language; plan.probe = probe; plan.ts = &rule;
    int64_t max_rounds = 1;
    for (int i = 0; i < n_clips; ++i) max_rounds = std::max<int64_t>(max_rounds, (n_samples[i] + tick - 1) / tick + 1);
    const int per_window = s->fb_set ? std::max(beam_size, s->fb.best_of) : beam_size;
    const size_t per_group = (size_t)(STT_GROUP / per_window);
    const int most = (int)std::min<size_t>((size_t)n_clips, per_group);
    RT_TRY(stt_group_reserve(s, most));
    RT_TRY(stt_beam_reserve(s, most * per_window));
    RT_TRY(stt_plan_begin(s, plan, n_clips));
    std::vector<SttFbWin> fb_group;
    if (s->fb_set) plan.fallback = &fb_group;
    // a prompt policy ("conditioning on previous text"): per clip the history - it starts as the initial prompt -
    // and the reset mark; a window's prompt is the history behind the mark, cut to its last stt_prompt_cap ids
    const bool prompted = s->pr_set;
    if (prompted) RT_TRY(stt_prompt_reserve(s, most, most * per_window));
    std::vector<std::vector<int32_t>> hist(prompted ? n_clips : 0, s->pr_initial), prompts;
    std::vector<size_t> mark(prompted ? n_clips : 0, 0);
    res.fb.assign(n_clips, {});
    res.ids.assign(n_clips, {}); res.segs.assign(n_clips, {}); res.wins.assign(n_clips, {});
    res.score.assign(n_clips, 0.f); res.lang_prob.assign(n_clips, 1.f); res.lang.assign(n_clips, 0);     // (round 0 fills both for every clip)
    std::vector<int64_t> off(n_clips, 0);
    std::vector<char> done(n_clips, 0);
    std::vector<double> sum(n_clips, 0.0), sum_all(n_clips, 0.0);
    std::vector<int64_t> count(n_clips, 0), count_all(n_clips, 0);
    const bool silence = o.no_speech_threshold == o.no_speech_threshold;
    std::vector<SttSpan> spans;
    std::vector<SttHyp> hyps;
    std::vector<SttWinInfo> info;
    std::vector<SttSeg> segs;
    for (int64_t round = 0; round < max_rounds; ++round) {
        spans.clear();
        for (int i = 0; i < n_clips; ++i)
            if (!done[i]) spans.push_back({i, n_samples[i] > 0 ? d_pcm[i] + off[i] : nullptr, std::min<int64_t>(win, n_samples[i] - off[i]), (uint32_t)(off[i] / tick)});
        if (spans.empty()) break;
        if (prompted) {
            prompts.assign(spans.size(), {});
            for (size_t k = 0; k < spans.size(); ++k) {
                const std::vector<int32_t>& hs = hist[spans[k].clip];
                const size_t from = std::max(mark[spans[k].clip], hs.size() - std::min(hs.size(), (size_t)stt_prompt_cap(c)));
                prompts[k].assign(hs.begin() + from, hs.end());
            }
        }
        for (size_t next = 0; next < spans.size(); next += per_group) {
            const int nW = (int)std::min(per_group, spans.size() - next);
            if (prompted) plan.prompt = prompts.data() + next;
            // a clip's language is fixed by its first window: round 0 detects, later rounds find it in d_clip_lang
            for (int b = 0; b < nW; ++b) plan.win_first[b] = round == 0 ? b : -1;
            RT_TRY(stt_run_group(s, spans.data() + next, nW, sr, beam_size, plan, hyps, info));
            for (int b = 0; b < nW; ++b) {
                const SttSpan& sp = spans[next + b];
                const int i = sp.clip;
                const SttHyp& h = hyps[b];
                if (round == 0) { res.lang[i] = info[b].lang; res.lang_prob[i] = info[b].lang_prob; }
                const float ns = info[b].no_speech;
                const float avg = h.score / (float)h.count;
                const bool silent = silence && ns > o.no_speech_threshold && (!(o.logprob_threshold == o.logprob_threshold) || avg < o.logprob_threshold);
                sum_all[i] += (double)h.score; count_all[i] += h.count;
                int advance = whole;
                if (!silent) {
                    sum[i] += (double)h.score; count[i] += h.count;
                    segs.clear();
                    advance = stt_seek_rule(h.ids, s->ts_begin, (int)std::min<int64_t>(whole, sp.n / tick), whole, segs);
                    const int64_t base = off[i] / tick;
                    for (const SttSeg& g : segs) {
                        res.segs[i].push_back({i, base + g.start, base + g.end, (int)g.ids.size()});
                        res.ids[i].insert(res.ids[i].end(), g.ids.begin(), g.ids.end());
                    }
                }
                // the history gains the window's closed segments, timestamps included - not a discarded tail, not a segment of no
                // duration or without a text id - and the mark moves behind them when conditioning is off or the chosen attempt ran
                // above the reset temperature.  A silent window leaves both as they are.
                int reset = 0;
                if (prompted && !silent) {
                    for (const SttSeg& g : segs)
                        if (g.start != g.end && !g.ids.empty()) hist[i].insert(hist[i].end(), g.raw.begin(), g.raw.end());
                    const float T = plan.fallback ? fb_group[b].temperature : 0.f;
                    if (!s->pr.condition_on_previous || T > s->pr.reset_on_temperature) { mark[i] = hist[i].size(); reset = 1; }
                }
                if (advance <= 0) advance = whole;                  // (a window that would not move its clip moves it by a whole window)
                res.wins[i].push_back({i, off[i], (int)h.ids.size(), h.score, ns, advance, prompted ? (int)prompts[next + b].size() : 0, reset});
                if (plan.fallback) res.fb[i].push_back(fb_group[b]);
                off[i] += (int64_t)advance * tick;
                if (off[i] >= n_samples[i]) done[i] = 1;
            }
        }
    }
    for (int i = 0; i < n_clips; ++i)
        res.score[i] = count[i] > 0 ? (float)(sum[i] / (double)count[i]) : (float)(sum_all[i] / (double)std::max<int64_t>(count_all[i], 1));
    return RT_OK;
}

// argument rules shared by the batched entry points: null for a clip with samples, a negative length
int stt_check_clips(const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips) {
    if (n_clips < 0 || (n_clips > 0 && (!d_pcm || !n_samples))) return RT_ERR_INVALID;
    for (int i = 0; i < n_clips; ++i)
        if (n_samples[i] < 0 || (n_samples[i] > 0 && !d_pcm[i])) return RT_ERR_INVALID;
    return RT_OK;
}

// The language requests of a call of `who` (null: none): -1 asks for detection - the probe pass then runs, as it does when `probe`
// comes in set - and any other id must be configured.  wants: what the probe serves in that entry point, for the user's message
int stt_check_languages(rt_stt* s, const char* who, const char* wants, const int32_t* h_req, int n_clips, bool& probe) {
    for (int i = 0; h_req && i < n_clips; ++i) {
        if (h_req[i] == -1) { probe = true; continue; }
        if (std::find(s->lang_ids.begin(), s->lang_ids.end(), h_req[i]) == s->lang_ids.end())
            return rt_fail(s->ctx, RT_ERR_INVALID, "%s: clip %d: language %d is neither -1 nor a configured id (rt_stt_set_languages)", who, i, h_req[i]);
    }
    if ((h_req || probe) && s->lang_ids.empty()) return rt_fail(s->ctx, RT_ERR_INVALID, "%s: %s asked of a handle without rt_stt_set_languages", who, wants);
    return RT_OK;
}


// ---------------------------------------------------------------------------------------------- token times (rt_stt_align)
// Frames of a window of n_in samples at rate sr ("word times"): half the log-mel frames of its resampled length
// (Resampler::n_out, restated so that nothing has to be designed first), at least 1, at most n_ctx.  One frame is 0.02 s.
int stt_align_frames(const rt_stt_config& c, int sr, int64_t n_in) {
    int64_t n16 = n_in;
    if (sr != c.sample_rate) {
        int a = sr, b = c.sample_rate;
        while (b) { const int t = a % b; a = b; b = t; }
        const int64_t L = c.sample_rate / a, M = sr / a;
        n16 = (n_in * L + M - 1) / M;
    }
    return (int)std::min<int64_t>(std::max<int64_t>(n16 / c.hop / 2, 1), c.n_ctx);
}

// The alignment side holds what `need` asks for (stt_reserve, as the beam path's)
int stt_align_reserve(rt_stt* s, const SttAlignNeed& need) {
    const SttAlignNeed& h = s->aln.has;
    if (h.rows >= need.rows && h.w >= need.w && h.m >= need.m && h.stats >= need.stats && h.trace >= need.trace && h.tab >= need.tab && h.arows >= need.arows) return RT_OK;
    SttAlignNeed n;
    n.rows = std::max(h.rows, need.rows); n.w = std::max(h.w, need.w); n.m = std::max(h.m, need.m); n.stats = std::max(h.stats, need.stats);
    n.trace = std::max(h.trace, need.trace); n.tab = std::max(h.tab, need.tab); n.arows = std::max(h.arows, need.arows);
    return stt_reserve(s, s->aln, [&](SttAlignBuf& nb) -> int {
        const rt_stt_config& c = s->cfg;
        RT_TRY(stt_alloc_work(s, nb.owned, n.rows, nb.work));
        RT_TRY(stt_alloc(s, nb.owned, n.rows, &nb.enc_last));
        RT_TRY(stt_alloc(s, nb.owned, (size_t)STT_ALIGN_CHUNK * c.d_model, &nb.xl)); RT_TRY(stt_alloc(s, nb.owned, (size_t)STT_ALIGN_CHUNK * c.d_model, &nb.xn));
        RT_TRY(stt_alloc(s, nb.owned, (size_t)STT_ALIGN_CHUNK * c.vocab, &nb.logits));
        RT_TRY(stt_alloc(s, nb.owned, n.w, &nb.W)); RT_TRY(stt_alloc(s, nb.owned, n.m, &nb.M)); RT_TRY(stt_alloc(s, nb.owned, n.arows, &nb.lp));
        RT_TRY(stt_alloc(s, nb.owned, n.stats, &nb.stats)); RT_TRY(stt_alloc(s, nb.owned, n.trace, &nb.trace));
        RT_TRY(stt_alloc(s, nb.owned, n.arows, &nb.frames)); RT_TRY(stt_alloc(s, nb.owned, n.tab, &nb.tab));
        hipLaunchKernelGGL(k_stt_fill_i32, dim3(64), dim3(256), 0, s->ctx->stream, nb.enc_last, (int)n.rows, c.n_ctx - 1, 0);
        RT_HIP(s->ctx, hipGetLastError());
        nb.has = n;
        return RT_OK;
    });
}

// One window of an rt_stt_align call: its samples, its text ids and the id position 1 of its prefix takes
struct SttAlignItem { SttSpan span; const int32_t* ids; int n; int32_t lang; };
// What rt_debug_stt_align_stages reads of a group (host memory; caps in floats): W [window][head][r_max][f_max] and M, window by window
struct SttAlignStages { float* h_W; size_t w_cap; float* h_M; size_t m_cap; int32_t r_max, f_max; };

// One group (1 .. STT_GROUP windows, every one with ids) through the four steps: front end and encoder; ONE teacher-forced pass over
// the rows [prefix + ids] of every window - stt_decode_tab's embedding and layers (stt_decode_tab_rows) with the capture argument set,
// and its tail (final LayerNorm, LM head) run here over the rows that predict a text id only, STT_ALIGN_CHUNK at a time: the logits of
// every row at once would be rows x vocab floats; the probabilities' normalisation, filter and head mean; the paths.  Row k of a window's alignment rows sits at
// position P - 1 + k and predicts token k of ids + [end-of-sequence]; the row whose input would be end-of-sequence is not fed.
// h_frames [sum (n + 1)], h_lp [sum n] (null: not wanted).  The group's uploads come first, while the stream is idle.
int stt_align_group(rt_stt* s, const SttAlignItem* it, int nW, int sr, int32_t* h_frames, float* h_lp, SttAlignStages* stages) {
    rt_ctx* ctx = s->ctx;
    const rt_stt_config& c = s->cfg;
    const int P = c.n_prefix, NH = (int)s->al_heads.size(), D = c.d_model;
    size_t M = 0, A = 0, L = 0, m_n = 0, trace_n = 0;
    int r_max = 0, f_max = 0;
    std::vector<int> F(nW);
    for (int b = 0; b < nW; ++b) {
        F[b] = stt_align_frames(c, sr, it[b].span.n);
        M += (size_t)P + it[b].n; A += (size_t)it[b].n + 1; L += it[b].n;
        r_max = std::max(r_max, it[b].n + 1); f_max = std::max(f_max, F[b]);
        m_n += (size_t)(it[b].n + 1) * F[b];
        trace_n += align_trace_words(it[b].n + 1, F[b]);
    }
    const int64_t head_stride = (int64_t)r_max * f_max;
    constexpr size_t WIN_WORDS = sizeof(AlignWin) / 4;
    static_assert(sizeof(AlignWin) % 8 == 0, "AlignWin is laid out in 64-bit units");
    // the tables of the group (32-bit words; the two 64-bit parts first)
    const size_t o_wins = 0, o_aout = o_wins + WIN_WORDS * nW, o_tok = o_aout + 2 * A, o_slot = o_tok + M, o_pos = o_slot + M, o_asrc = o_pos + M, o_aslot = o_asrc + A,
                 o_afr = o_aslot + A, o_lrow = o_afr + A, o_ltok = o_lrow + L, tab_n = o_ltok + L;
    SttAlignNeed need;
    need.rows = M; need.w = (size_t)nW * NH * head_stride; need.m = m_n; need.stats = (size_t)nW * NH * f_max * 2; need.trace = trace_n; need.tab = tab_n; need.arows = A;
    RT_TRY(stt_group_reserve(s, nW));
    RT_TRY(stt_align_reserve(s, need));
    SttAlignBuf& ab = s->aln;
    std::vector<int32_t>& h = s->h_aln;
    h.assign(tab_n, 0);
    std::vector<SttSpan> spans(nW);
    {
        std::vector<AlignWin> wins(nW);
        std::vector<int64_t> aout(A);
        size_t row = 0, a = 0, l = 0, m_off = 0, t_off = 0;
        for (int b = 0; b < nW; ++b) {
            spans[b] = it[b].span;
            const int n = it[b].n;
            wins[b] = AlignWin{n + 1, F[b], (int64_t)b * NH * head_stride, (int64_t)m_off, (int64_t)a, (int64_t)t_off};
            m_off += (size_t)(n + 1) * F[b];
            t_off += align_trace_words(n + 1, F[b]);
            for (int i = 0; i < P + n; ++i, ++row) {
                h[o_tok + row] = i < P ? ((i == 1 && P > 1) ? it[b].lang : c.prefix[i]) : it[b].ids[i - P];
                h[o_slot + row] = b; h[o_pos + row] = i;
                if (i < P - 1) continue;
                const int k = i - (P - 1);                 // alignment row k: predicts ids[k], the last one end-of-sequence
                h[o_asrc + a] = (int32_t)row; h[o_aslot + a] = b; h[o_afr + a] = F[b];
                aout[a] = wins[b].w_off + (int64_t)k * f_max;
                ++a;
                if (k < n) { h[o_lrow + l] = (int32_t)row; h[o_ltok + l] = it[b].ids[k]; ++l; }
            }
        }
        memcpy(h.data() + o_wins, wins.data(), sizeof(AlignWin) * nW);
        memcpy(h.data() + o_aout, aout.data(), 8 * A);
    }
    RT_HIP(ctx, hipMemcpyAsync(ab.tab, h.data(), tab_n * 4, hipMemcpyHostToDevice, ctx->stream));
    const int32_t* tab = ab.tab;
    const AlignWin* d_wins = reinterpret_cast<const AlignWin*>(tab + o_wins);
    RT_TRY(stt_features_group(s, spans.data(), nW, sr));
    for (int b = 0; b < nW; ++b)      // (stt_align_frames restates the resampled length: held against what the front end made of the window)
        if (F[b] != (int)std::min<int64_t>(std::max<int64_t>(s->h_wins[b].n16 / c.hop / 2, 1), c.n_ctx))
            return rt_fail(ctx, RT_ERR_STATE, "align: window %d: %d frames planned, the front end holds %lld samples", b, F[b], (long long)s->h_wins[b].n16);
    RT_TRY(stt_encode(s, s->grp.enc, nW));
    // the teacher-forced pass
    const KvCache& cross = s->grp.enc.cross_kv;
    SttSlot* emb = stt_find(s, "dec.tok");
    const SttWork& k = ab.work;
    SttCapture cap{AlignRows{tab + o_asrc, tab + o_aslot, tab + o_afr, reinterpret_cast<const int64_t*>(tab + o_aout)}, (int)A, s->al_layers.data(), head_stride, ab.W};
    RT_TRY(stt_decode_tab_rows(s, k, s->grp.dec.kv, cross, (int)M, tab + o_tok, tab + o_slot, tab + o_pos, tab + o_slot, ab.enc_last, &cap));
    // token log-probabilities: log_softmax over the text ids [0, end-of-sequence) at the token a row predicts
    for (size_t at = 0; at < L; at += STT_ALIGN_CHUNK) {
        const int n = (int)std::min<size_t>(STT_ALIGN_CHUNK, L - at);
        hipLaunchKernelGGL(k_stt_take_rows, dim3(n), dim3(64), 0, ctx->stream, k.x, tab + o_lrow + at, D, ab.xl);
        RT_HIP(ctx, hipGetLastError());
        RT_TRY(stt_ln(s, ab.xl, D, n, SVEC(s, "dec.ln_w"), SVEC(s, "dec.ln_b"), ab.xn));
        RT_TRY(stt_gemm(s, ab.xn, n, emb->pw, nullptr, ACT_NONE, nullptr, ab.logits));
        RT_TRY(launch_align_logprob(ctx, ab.logits, c.vocab, n, tab + o_ltok + at, c.eos_id, ab.lp + at));
    }
    {
        SttAlignSpan span(s, 1);
        RT_TRY(launch_align_matrix(ctx, ab.W, d_wins, nW, NH, head_stride, f_max, r_max, f_max, s->al_width, ab.stats, ab.M));
    }
    {
        SttAlignSpan span(s, 2);
        RT_TRY(launch_align_dtw(ctx, ab.M, d_wins, nW, r_max, f_max, ab.trace, -1, ab.frames));
    }
    s->h_aln_frames.resize(A); s->h_aln_lp.resize(std::max<size_t>(L, 1));
    RT_HIP(ctx, hipMemcpyAsync(s->h_aln_frames.data(), ab.frames, A * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (L) RT_HIP(ctx, hipMemcpyAsync(s->h_aln_lp.data(), ab.lp, L * 4, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    stt_align_clock_collect(s);
    if (h_frames) std::copy(s->h_aln_frames.begin(), s->h_aln_frames.end(), h_frames);
    if (h_lp) std::copy(s->h_aln_lp.begin(), s->h_aln_lp.begin() + L, h_lp);
    if (stages) {
        stages->r_max = r_max; stages->f_max = f_max;
        if (need.w > stages->w_cap || m_n > stages->m_cap) return rt_fail(ctx, RT_ERR_LENGTH, "align stages: %zu and %zu floats, room for %zu and %zu", need.w, m_n, stages->w_cap, stages->m_cap);
        // (the capture writes rows <= n, t < F of every window and nothing reads the other cells: the copy shows them as zeros)
        RT_HIP(ctx, hipMemcpy(stages->h_W, ab.W, need.w * 4, hipMemcpyDeviceToHost));
        RT_HIP(ctx, hipMemcpy(stages->h_M, ab.M, m_n * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < nW; ++b)
            for (int hh = 0; hh < NH; ++hh)
                for (int r = 0; r < r_max; ++r)
                    for (int t = 0; t < f_max; ++t)
                        if (r > it[b].n || t >= F[b]) stages->h_W[((size_t)b * NH + hh) * head_stride + (size_t)r * f_max + t] = 0.f;
    }
    return RT_OK;
}

// The argument rules of rt_stt_align, all of them before the first launch, and the call's windows as items
int stt_align_check(rt_stt* s, const char* who, const float* const* d_pcm, const int64_t* n_samples, int32_t n_windows, int32_t sr, const int32_t* h_text_ids,
                    const int32_t* h_text_offsets, const int32_t* h_language, std::vector<SttAlignItem>& items) {
    rt_ctx* ctx = s->ctx;
    const rt_stt_config& c = s->cfg;
    if (n_windows < 0 || sr < 1000 || stt_check_clips(d_pcm, n_samples, n_windows) || (n_windows > 0 && !h_text_offsets) || (n_windows > 0 && h_text_offsets[0] != 0))
        return rt_fail(ctx, RT_ERR_INVALID, "%s: bad argument", who);
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "%s: not finalized", who);
    if (s->al_heads.empty()) return rt_fail(ctx, RT_ERR_INVALID, "%s: the handle has no alignment heads (rt_stt_set_alignment)", who);
    bool probe = false;
    RT_TRY(stt_check_languages(s, who, "languages", h_language, n_windows, probe));
    if (probe) return rt_fail(ctx, RT_ERR_INVALID, "%s: a window's language must be given (-1, detection, is not offered here: detect with rt_stt_detect_language)", who);
    const int room = c.n_text_ctx - c.n_prefix - 1;
    items.clear();
    for (int w = 0; w < n_windows; ++w) {
        const int64_t n = (int64_t)h_text_offsets[w + 1] - h_text_offsets[w];
        if (n < 0 || (n > 0 && !h_text_ids)) return rt_fail(ctx, RT_ERR_INVALID, "%s: window %d: text offsets must not decrease", who, w);
        if (n > room) return rt_fail(ctx, RT_ERR_LENGTH, "%s: length: window %d has %lld text ids, a text context of %d behind %d forced ids takes %d", who, w, (long long)n, c.n_text_ctx, c.n_prefix, room);
        if (n_samples[w] > (int64_t)c.chunk_seconds * sr)
            return rt_fail(ctx, RT_ERR_LENGTH, "%s: length: window %d has %lld samples, one window is at most %d s", who, w, (long long)n_samples[w], c.chunk_seconds);
        for (int64_t i = 0; i < n; ++i) {
            const int32_t id = h_text_ids[h_text_offsets[w] + i];
            if (id < 0 || id >= c.vocab) return rt_fail(ctx, RT_ERR_INVALID, "%s: window %d: id %d outside the vocabulary of %d", who, w, id, c.vocab);
            // (a token's log-probability is taken over the text ids [0, end-of-sequence): a special or timestamp id has none)
            if (id >= c.eos_id) return rt_fail(ctx, RT_ERR_INVALID, "%s: window %d: id %d is not a text id (end-of-sequence is %d)", who, w, id, c.eos_id);
        }
        items.push_back({SttSpan{w, n_samples[w] > 0 ? d_pcm[w] : nullptr, n_samples[w]}, h_text_ids ? h_text_ids + h_text_offsets[w] : nullptr, (int)n,
                         h_language ? h_language[w] : (c.n_prefix > 1 ? c.prefix[1] : 0)});
    }
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_stt_create(rt_ctx* ctx, const rt_stt_config* cfg, rt_stt** out) {
    if (!ctx || !cfg || !out) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_create: null argument");
    *out = nullptr;
    const rt_stt_config& c = *cfg;
    const int d = c.heads > 0 ? c.d_model / c.heads : 0;
    if (c.d_model < 16 || c.d_model % 8 || c.heads < 1 || c.d_model % c.heads || (d != 32 && d != 64 && d != 128) || c.ffn % 8 || c.n_mels % 8 ||
        c.enc_layers < 1 || c.dec_layers < 1 || c.n_ctx < 2 || c.n_text_ctx < 2 || c.vocab < 2 || c.n_fft < 16 || c.n_fft % 2 || c.hop < 1 ||
        c.sample_rate < 1000 || c.chunk_seconds < 1 || (int64_t)c.chunk_seconds * c.sample_rate / c.hop != 2 * (int64_t)c.n_ctx || c.n_prefix < 1 ||
        c.n_prefix > 8 || c.n_begin_suppress < 0 || c.n_begin_suppress > 4 || c.eos_id < 0 || c.eos_id >= c.vocab || c.max_new_tokens < 1 ||
        c.n_prefix + c.max_new_tokens > c.n_text_ctx || c.n_fft > 2048)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_create: unsupported configuration (head_dim in {32,64,128}, widths %% 8, 2 n_ctx = frames of one chunk)");
    for (int i = 0; i < c.n_prefix; ++i)      // (forced ids index the embedding table)
        if (c.prefix[i] < 0 || c.prefix[i] >= c.vocab) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_create: forced prefix id %d outside the vocabulary of %d", c.prefix[i], c.vocab);
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    rt_stt* s = new rt_stt();
    s->ctx = ctx;
    s->cfg = c;
    stt_declare(s);
    *out = s;
    return RT_OK;
}

int rt_stt_destroy(rt_stt* s) {
    if (!s) return RT_OK;
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& sl : s->slots) { if (sl.raw) (void)hipFree(sl.raw); if (sl.raw2) (void)hipFree(sl.raw2); }
    for (auto* owned : {&s->owned, &s->grp.owned, &s->beam.owned, &s->prm.owned, &s->aln.owned})
        for (void* p : *owned) (void)hipFree(p);
    if (s->rs.d_h) (void)hipFree(s->rs.d_h);
    delete s;
    return RT_OK;
}

int rt_stt_tensor_count(rt_stt* s) { return s ? (int)s->slots.size() : -1; }

int rt_stt_tensor_info(rt_stt* s, int32_t index, char* name, size_t name_cap, int64_t* shape2, int32_t* kind) {
    if (!s || index < 0 || index >= (int)s->slots.size()) return RT_ERR_INVALID;
    const SttSlot& sl = s->slots[index];
    if (name && name_cap) snprintf(name, name_cap, "%s", sl.name.c_str());
    if (shape2) { shape2[0] = sl.rows; shape2[1] = sl.cols; }
    if (kind) *kind = sl.kind;
    return RT_OK;
}

int rt_stt_set_tensor(rt_stt* s, const char* name, const void* data, int32_t dtype, int64_t rows, int64_t cols, int32_t on_device) {
    if (!s || !name || !data) return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_stt_set_tensor: null argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    SttSlot* sl = stt_find(s, name);
    if (!sl) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_tensor: unknown tensor '%s'", name);
    if (sl->rows * sl->cols != rows * cols || (sl->kind != S_VEC && (sl->rows != rows || sl->cols != cols)))
        return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_tensor: '%s' expects [%lld, %lld], got [%lld, %lld]", name, (long long)sl->rows, (long long)sl->cols,
                       (long long)rows, (long long)cols);
    if (sl->kind != S_VEC && dtype != RT_DTYPE_BF16) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_tensor: '%s' must be bf16", name);
    const int64_t n = rows * cols;
    const size_t esz = dtype == RT_DTYPE_BF16 ? 2 : 4;
    const void* d_src = data;
    if (!on_device) {
        void* stage = nullptr;
        RT_TRY(rt_ctx_scratch(ctx, (size_t)n * esz, &stage));
        RT_HIP(ctx, hipMemcpyAsync(stage, data, (size_t)n * esz, hipMemcpyHostToDevice, ctx->stream));
        d_src = stage;
    }
    if (sl->raw) { RT_HIP(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(sl->raw); sl->raw = nullptr; }
    if (sl->raw2) { (void)hipFree(sl->raw2); sl->raw2 = nullptr; }
    if (sl->kind == S_GEMM || sl->kind == S_TABLE) {
        void** packed = sl->kind == S_GEMM ? &sl->raw : &sl->raw2;
        RT_HIP(ctx, hipMalloc(packed, packed_bytes((int)rows, (int)cols)));
        RT_TRY(launch_pack_weight(ctx, (const bf16_t*)d_src, (int)rows, (int)cols, (bf16_t*)*packed, &sl->pw));
        if (sl->kind == S_TABLE) {
            RT_HIP(ctx, hipMalloc(&sl->raw, (size_t)n * 2));
            RT_HIP(ctx, hipMemcpyAsync(sl->raw, d_src, (size_t)n * 2, hipMemcpyDeviceToDevice, ctx->stream));
            sl->tbl = (bf16_t*)sl->raw;
        }
    } else {
        RT_HIP(ctx, hipMalloc(&sl->raw, (size_t)n * 4));
        sl->vec = (float*)sl->raw;
        if (dtype == RT_DTYPE_F32) RT_HIP(ctx, hipMemcpyAsync(sl->raw, d_src, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        else hipLaunchKernelGGL(k_stt_bf16_to_f32, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)), dim3(256), 0, ctx->stream, (const bf16_t*)d_src, n, sl->vec);
        RT_HIP(ctx, hipGetLastError());
    }
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    sl->set = true;
    return RT_OK;
}

int rt_stt_finalize(rt_stt* s) {
    if (!s) return RT_ERR_INVALID;
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_stt_finalize: already finalized");
    for (auto& sl : s->slots)
        if (!sl.set) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_finalize: tensor '%s' was never set", sl.name.c_str());
    const rt_stt_config& c = s->cfg;
    std::vector<double> tc(c.n_fft), ts(c.n_fft);
    for (int n = 0; n < c.n_fft; ++n) { tc[n] = std::cos(2.0 * M_PI * n / c.n_fft); ts[n] = std::sin(2.0 * M_PI * n / c.n_fft); }
    RT_TRY(stt_alloc(s, s->owned, (size_t)c.n_fft, &s->d_twc)); RT_TRY(stt_alloc(s, s->owned, (size_t)c.n_fft, &s->d_tws));
    RT_HIP(ctx, hipMemcpy(s->d_twc, tc.data(), c.n_fft * 8, hipMemcpyHostToDevice));
    RT_HIP(ctx, hipMemcpy(s->d_tws, ts.data(), c.n_fft * 8, hipMemcpyHostToDevice));
    s->d_window = SVEC(s, "fe.window");
    s->d_melT = SVEC(s, "fe.melT");
    RT_TRY(stt_group_reserve(s, 1));                                 // a model that does not fit fails here, and the first call pays no allocation
    // suppression mask: bit 0 = never (ids >= suppress_from except end-of-sequence), bit 1 = not as the first generated token
    std::vector<uint8_t> mask(c.vocab, 0);
    for (int i = 0; i < c.vocab; ++i)
        if (c.suppress_from > 0 && i >= c.suppress_from && i != c.eos_id) mask[i] |= 1;
    for (int i = 0; i < c.n_begin_suppress; ++i)
        if (c.begin_suppress[i] >= 0 && c.begin_suppress[i] < c.vocab) mask[c.begin_suppress[i]] |= 2;
    for (int32_t id : s->suppress_ids)
        if (id >= 0 && id < c.vocab && id != c.eos_id) mask[id] |= 1;
    RT_TRY(stt_alloc(s, s->owned, (size_t)c.vocab, &s->d_mask));
    RT_HIP(ctx, hipMemcpy(s->d_mask, mask.data(), c.vocab, hipMemcpyHostToDevice));
    if (!s->lang_ids.empty()) {                                      // rt_stt_set_languages: one group's worth of the probe's buffers
        RT_TRY(stt_alloc(s, s->owned, s->lang_ids.size(), &s->d_lang_ids));
        RT_HIP(ctx, hipMemcpy(s->d_lang_ids, s->lang_ids.data(), s->lang_ids.size() * 4, hipMemcpyHostToDevice));
        RT_TRY(stt_alloc(s, s->owned, (size_t)STT_GROUP, &s->d_sot));
        RT_TRY(stt_alloc(s, s->owned, (size_t)4 * STT_GROUP, &s->d_probe));
        RT_TRY(stt_alloc(s, s->owned, (size_t)2 * STT_GROUP, &s->d_win_meta));
        RT_HIP(ctx, hipMemsetAsync(s->d_probe, 0, (size_t)4 * STT_GROUP * 4, ctx->stream));
        hipLaunchKernelGGL(k_stt_fill_i32, dim3(1), dim3(64), 0, ctx->stream, s->d_sot, STT_GROUP, c.prefix[0], 0);
        RT_HIP(ctx, hipGetLastError());
    }
    if (!s->lang_ids.empty() || s->ts_begin > 0) RT_TRY(stt_alloc(s, s->owned, (size_t)STT_GROUP * c.n_prefix, &s->d_win_prefix));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->finalized = true;
    return RT_OK;
}

int rt_stt_log_mel(rt_stt* s, const float* d_pcm, int64_t n_samples, int32_t sample_rate, float* d_mel) {
    if (!s || !d_mel || n_samples < 0 || (n_samples > 0 && !d_pcm) || sample_rate < 1000) return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_stt_log_mel: bad argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_stt_log_mel: not finalized");
    const SttSpan clip{0, d_pcm, n_samples};                         // (uncut: the resampler's taps at the end of the chunk see the samples behind it)
    RT_TRY(stt_group_reserve(s, 1));
    RT_TRY(stt_features_group(s, &clip, 1, sample_rate));
    RT_HIP(ctx, hipMemcpyAsync(d_mel, s->grp.enc.mel, (size_t)2 * s->cfg.n_ctx * s->cfg.n_mels * 4, hipMemcpyDeviceToDevice, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_stt_encode(rt_stt* s, const float* d_pcm, int64_t n_samples, int32_t sample_rate, float* d_states) {
    if (!s || !d_states || n_samples < 0 || (n_samples > 0 && !d_pcm) || sample_rate < 1000) return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_stt_encode: bad argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_stt_encode: not finalized");
    const SttSpan clip{0, d_pcm, n_samples};                         // (uncut, as rt_stt_log_mel)
    RT_TRY(stt_group_reserve(s, 1));
    RT_TRY(stt_features_group(s, &clip, 1, sample_rate));
    RT_TRY(stt_encode(s, s->grp.enc, 1));
    RT_HIP(ctx, hipMemcpyAsync(d_states, s->grp.enc.out, (size_t)s->cfg.n_ctx * s->cfg.d_model * 4, hipMemcpyDeviceToDevice, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_stt_set_suppress(rt_stt* s, const int32_t* h_ids, int32_t n) {
    if (!s || n < 0 || (n > 0 && !h_ids)) return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_stt_set_suppress: bad argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    if (s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_stt_set_suppress: call before rt_stt_finalize (the mask is built there)");
    s->suppress_ids.assign(h_ids, h_ids + n);
    return RT_OK;
}

// Audio longer than one chunk is transcribed window by window (consecutive chunk_seconds windows of the INPUT, each a row of the
// resampler, the log-mel front-end, the encoder and the greedy decode behind the forced prefix) and the ids are concatenated:
// the whole clip is heard, as with the reference's transcribers (faster-whisper walks 30-s windows, stt_validator.py:133-141),
// though not at their seek positions - those follow timestamp tokens, which the forced <|notimestamps|> prefix rules out.
int rt_stt_transcribe(rt_stt* s, const float* d_pcm, int64_t n_samples, int32_t sample_rate, int32_t* h_tokens, int32_t max_tokens, int32_t* h_n_tokens,
                      float* d_first_logits) {
    if (!s || !h_tokens || !h_n_tokens || max_tokens < 1 || n_samples < 0 || (n_samples > 0 && !d_pcm) || sample_rate < 1000)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_stt_transcribe: bad argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_stt_transcribe: not finalized");
    return stt_transcribe_greedy(s, &d_pcm, &n_samples, 1, sample_rate, h_tokens, max_tokens, h_n_tokens, d_first_logits);
}

// The windows of all clips are the rows of the batch (stt_transcribe_greedy): per clip what rt_stt_transcribe gives for it alone
int rt_stt_transcribe_batch(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips, int32_t sample_rate, int32_t* h_tokens,
                            int32_t max_tokens_per_clip, int32_t* h_n_tokens) {
    if (!s || max_tokens_per_clip < 1 || sample_rate < 1000 || stt_check_clips(d_pcm, n_samples, n_clips) || (n_clips > 0 && (!h_tokens || !h_n_tokens)))
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_stt_transcribe_batch: bad argument");
    if (n_clips == 0) return RT_OK;
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_stt_transcribe_batch: not finalized");
    return stt_transcribe_greedy(s, d_pcm, n_samples, n_clips, sample_rate, h_tokens, max_tokens_per_clip, h_n_tokens, nullptr);
}

// As rt_stt_transcribe_batch, decoded by beam search: floor(STT_GROUP / beam_size) windows make a group, whose decoder rows are
// windows x beams.  Every window is decoded (a clip's score counts all of its windows); max_tokens cuts the joined ids.
int rt_stt_transcribe_beam(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips, int32_t sample_rate, int32_t beam_size,
                           int32_t* h_tokens, int32_t max_tokens, int32_t* h_n_tokens, float* h_scores) {
    if (!s || max_tokens < 1 || sample_rate < 1000 || beam_size < 1 || beam_size > STT_BEAM_MAX || stt_check_clips(d_pcm, n_samples, n_clips) ||
        (n_clips > 0 && (!h_tokens || !h_n_tokens)))
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_stt_transcribe_beam: bad argument (beam_size 1 .. %d)", STT_BEAM_MAX);
    if (n_clips == 0) return RT_OK;
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_stt_transcribe_beam: not finalized");
    std::vector<SttSpan> all;
    stt_cut(s->cfg, sample_rate, d_pcm, n_samples, n_clips, all);
    return stt_transcribe_beam(s, all, n_clips, sample_rate, beam_size, h_tokens, max_tokens, h_n_tokens, h_scores, nullptr);
}

int rt_stt_set_languages(rt_stt* s, const int32_t* h_lang_ids, int32_t n, int32_t no_speech_id) {
    if (!s || !h_lang_ids || n < 1 || n > STT_LANG_MAX) return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_stt_set_languages: bad argument (1 .. %d ids)", STT_LANG_MAX);
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    if (s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_stt_set_languages: call before rt_stt_finalize");
    const rt_stt_config& c = s->cfg;
    if (c.n_prefix < 2) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_languages: the forced prefix has no language position (%d entries)", c.n_prefix);
    if (no_speech_id < 0 || no_speech_id >= c.vocab) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_languages: no-speech id %d outside the vocabulary of %d", no_speech_id, c.vocab);
    bool own = false;
    for (int i = 0; i < n; ++i) {
        if (h_lang_ids[i] < 0 || h_lang_ids[i] >= c.vocab) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_languages: language id %d outside the vocabulary of %d", h_lang_ids[i], c.vocab);
        own = own || h_lang_ids[i] == c.prefix[1];
    }
    if (!own) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_languages: position 1 of the configured prefix (%d) is not among the language ids", c.prefix[1]);
    s->lang_ids.assign(h_lang_ids, h_lang_ids + n);
    s->no_speech_id = no_speech_id;
    return RT_OK;
}

int rt_stt_detect_language(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips, int32_t sample_rate, int32_t* h_lang, float* h_lang_prob,
                           float* h_no_speech) {
    if (!s || sample_rate < 1000 || stt_check_clips(d_pcm, n_samples, n_clips) || (n_clips > 0 && !h_lang))
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_stt_detect_language: bad argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_stt_detect_language: not finalized");
    if (s->lang_ids.empty()) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_detect_language: the handle has no languages (rt_stt_set_languages)");
    if (n_clips == 0) return RT_OK;
    std::vector<SttSpan> all;
    stt_cut(s->cfg, sample_rate, d_pcm, n_samples, n_clips, all, true);
    RT_TRY(stt_group_reserve(s, std::min(n_clips, STT_GROUP)));
    SttGroup& w = s->grp;
    s->h_probe.resize(4 * STT_GROUP);
    for (int next = 0; next < n_clips; next += STT_GROUP) {
        const int nW = std::min(STT_GROUP, n_clips - next);
        RT_TRY(stt_features_group(s, all.data() + next, nW, sample_rate));
        RT_TRY(stt_encode(s, w.enc, nW));
        RT_TRY(stt_probe_pass(s, w.dec, w.step_slot, w.step_pos, nW));      // on the greedy decoder side: position 0 of slot b
        RT_HIP(ctx, hipMemcpyAsync(s->h_probe.data(), s->d_probe, 3 * STT_GROUP * 4, hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const float* pf = (const float*)s->h_probe.data();
        for (int b = 0; b < nW; ++b) {
            h_lang[next + b] = s->h_probe[b];
            if (h_lang_prob) h_lang_prob[next + b] = pf[STT_GROUP + b];
            if (h_no_speech) h_no_speech[next + b] = pf[2 * STT_GROUP + b];
        }
    }
    return RT_OK;
}

int rt_stt_transcribe_ex(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips, int32_t sample_rate, const rt_stt_decode_opts* opts,
                         rt_stt_decode_out* out) {
    if (!s || !opts || !out || opts->max_tokens < 1 || sample_rate < 1000 || opts->beam_size < 1 || opts->beam_size > STT_BEAM_MAX ||
        stt_check_clips(d_pcm, n_samples, n_clips) || (n_clips > 0 && (!out->h_tokens || !out->h_n_tokens)) || out->window_cap < 0)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_stt_transcribe_ex: bad argument (beam_size 1 .. %d)", STT_BEAM_MAX);
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_stt_transcribe_ex: not finalized");
    out->n_windows = 0;
    if (n_clips == 0) return RT_OK;
    SttReport rep;
    rep.h_req = opts->h_language;
    rep.h_lang = out->h_language; rep.h_lang_prob = out->h_language_prob;
    rep.win_clip = out->h_win_clip; rep.win_n_ids = out->h_win_n_ids; rep.win_logprob = out->h_win_logprob; rep.win_no_speech = out->h_win_no_speech;
    rep.probe = rep.win_no_speech != nullptr || (s->fb_set && s->fb.no_speech_threshold == s->fb.no_speech_threshold);
    RT_TRY(stt_check_languages(s, "rt_stt_transcribe_ex", "languages or no-speech probabilities", rep.h_req, n_clips, rep.probe));
    std::vector<SttSpan> all;
    stt_cut(s->cfg, sample_rate, d_pcm, n_samples, n_clips, all);
    s->fb_report.clear();                                            // (rt_stt_fallback_report speaks of the last call under a policy)
    const bool per_window = rep.win_clip || rep.win_n_ids || rep.win_logprob || rep.win_no_speech;
    if (per_window && (size_t)out->window_cap < all.size())
        return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_transcribe_ex: %zu windows, room for %d", all.size(), out->window_cap);
    const int rc = stt_transcribe_beam(s, all, n_clips, sample_rate, opts->beam_size, out->h_tokens, opts->max_tokens, out->h_n_tokens, out->h_scores, &rep);
    if (rc != RT_OK) { s->fb_report.clear(); return rc; }           // (a failed call - the ratio callback's, say - leaves no partial report)
    out->n_windows = (int32_t)all.size();
    return RT_OK;
}

int rt_stt_set_timestamps(rt_stt* s, int32_t timestamp_begin, int32_t n_timestamps) {
    if (!s) return RT_ERR_INVALID;
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    if (s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_stt_set_timestamps: call before rt_stt_finalize");
    const rt_stt_config& c = s->cfg;
    if (timestamp_begin < 1 || n_timestamps < 2 || (int64_t)timestamp_begin + n_timestamps > c.vocab)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_timestamps: the vocabulary of %d does not hold timestamp ids %d .. %lld", c.vocab, timestamp_begin,
                       (long long)timestamp_begin + n_timestamps - 1);
    if (c.n_prefix < 2 || c.prefix[c.n_prefix - 1] != timestamp_begin - 1)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_timestamps: the configured prefix does not end in <|notimestamps|> = %d", timestamp_begin - 1);
    if (c.eos_id >= timestamp_begin - 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_timestamps: end-of-sequence %d is not below <|notimestamps|>", c.eos_id);
    s->ts_begin = timestamp_begin;
    s->ts_count = n_timestamps;
    return RT_OK;
}

// Clips of any length by timestamps and seek: stt_transcribe_seek computes the whole result on the host,
// then it is written out under the caps - nothing past one; RT_ERR_LENGTH with the counts a repeat needs when one is too small.
int rt_stt_transcribe_seek(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips, int32_t sample_rate, const rt_stt_seek_opts* opts,
                           rt_stt_seek_out* out) {
    if (!s || !opts || !out || opts->max_tokens < 1 || sample_rate < 1000 || opts->beam_size < 1 || opts->beam_size > STT_BEAM_MAX ||
        stt_check_clips(d_pcm, n_samples, n_clips) || (n_clips > 0 && (!out->h_tokens || !out->h_n_tokens)) || out->segment_cap < 1 || out->window_cap < 1 ||
        opts->max_initial_timestamp_index < -1)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_stt_transcribe_seek: bad argument (beam_size 1 .. %d, caps >= 1)", STT_BEAM_MAX);
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_stt_transcribe_seek: not finalized");
    if (s->ts_begin <= 0) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_transcribe_seek: the handle has no timestamp ids (rt_stt_set_timestamps)");
    out->n_segments = out->n_windows = out->max_clip_tokens = 0;
    if (n_clips == 0) return RT_OK;
    const bool silence = opts->no_speech_threshold == opts->no_speech_threshold;
    bool probe = out->h_win_no_speech != nullptr || silence || (s->fb_set && s->fb.no_speech_threshold == s->fb.no_speech_threshold);
    RT_TRY(stt_check_languages(s, "rt_stt_transcribe_seek", "languages, no-speech probabilities or the silence rule", opts->h_language, n_clips, probe));
    SttSeekResult res;
    s->fb_report.clear();
    s->pr_report.clear();
    RT_TRY(stt_transcribe_seek(s, d_pcm, n_samples, n_clips, sample_rate, *opts, probe, res));
    const double tick_s = (double)(int64_t)(0.02 * (double)sample_rate) / (double)sample_rate;
    int64_t n_seg = 0, n_win = 0;
    for (int i = 0; i < n_clips; ++i) {
        const int n_ids = (int)res.ids[i].size();
        out->max_clip_tokens = std::max(out->max_clip_tokens, n_ids);
        out->h_n_tokens[i] = std::min(n_ids, opts->max_tokens);
        std::copy(res.ids[i].begin(), res.ids[i].begin() + out->h_n_tokens[i], out->h_tokens + (size_t)i * opts->max_tokens);
        if (out->h_scores) out->h_scores[i] = res.score[i];
        if (out->h_language) out->h_language[i] = res.lang[i];
        if (out->h_language_prob) out->h_language_prob[i] = res.lang_prob[i];
        for (const SttSeekSeg& g : res.segs[i]) {
            const int64_t at = n_seg++;
            if (at >= out->segment_cap) continue;
            if (out->h_seg_clip) out->h_seg_clip[at] = i;
            if (out->h_seg_start_tick) out->h_seg_start_tick[at] = (int32_t)g.start_tick;
            if (out->h_seg_end_tick) out->h_seg_end_tick[at] = (int32_t)g.end_tick;
            if (out->h_seg_start) out->h_seg_start[at] = (float)((double)g.start_tick * tick_s);
            if (out->h_seg_end) out->h_seg_end[at] = (float)((double)g.end_tick * tick_s);
            if (out->h_seg_n_ids) out->h_seg_n_ids[at] = g.n_ids;
        }
        if (s->fb_set) s->fb_report.insert(s->fb_report.end(), res.fb[i].begin(), res.fb[i].end());
        for (const SttSeekWin& w : res.wins[i]) {
            if (s->pr_set) s->pr_report.push_back({w.prompt_len, w.reset});
            const int64_t at = n_win++;
            if (at >= out->window_cap) continue;
            if (out->h_win_clip) out->h_win_clip[at] = i;
            if (out->h_win_offset) out->h_win_offset[at] = w.off;
            if (out->h_win_n_ids) out->h_win_n_ids[at] = w.n_ids;
            if (out->h_win_logprob) out->h_win_logprob[at] = w.logprob;
            if (out->h_win_no_speech) out->h_win_no_speech[at] = w.no_speech;
            if (out->h_win_advance) out->h_win_advance[at] = w.advance;
        }
    }
    out->n_segments = (int32_t)n_seg;
    out->n_windows = (int32_t)n_win;
    if (n_seg > out->segment_cap || n_win > out->window_cap)
        return rt_fail(ctx, RT_ERR_LENGTH, "rt_stt_transcribe_seek: %lld segments and %lld windows, room for %d and %d", (long long)n_seg, (long long)n_win,
                       out->segment_cap, out->window_cap);
    return RT_OK;
}

int rt_stt_set_fallback(rt_stt* s, const rt_stt_fallback* f) {
    if (!s) return RT_ERR_INVALID;
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_stt_set_fallback: call after rt_stt_finalize");
    if (!f) { s->fb_set = false; s->fb = rt_stt_fallback{}; return RT_OK; }
    if (f->n_temperatures < 1 || f->n_temperatures > 8 || f->best_of < 1 || f->best_of > STT_BEAM_MAX)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_fallback: n_temperatures %d and best_of %d must lie in 1 .. 8", f->n_temperatures, f->best_of);
    for (int t = 0; t < f->n_temperatures; ++t) {
        const float T = f->temperatures[t];
        if (!(T >= 0.f) || std::isinf(T) || (t > 0 && !(T > f->temperatures[t - 1])))
            return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_fallback: temperature %d (%g) is negative, not finite or not above the one before it", t, (double)T);
    }
    if (f->compression_ratio_threshold == f->compression_ratio_threshold && !f->ratio)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_fallback: a compression_ratio_threshold needs the ratio callback");
    if (f->no_speech_threshold == f->no_speech_threshold && s->lang_ids.empty())
        return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_fallback: a no_speech_threshold needs a handle with rt_stt_set_languages");
    s->fb = *f;
    s->fb_set = true;
    return RT_OK;
}

int rt_stt_set_prompt(rt_stt* s, const rt_stt_prompt* p) {
    if (!s) return RT_ERR_INVALID;
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_stt_set_prompt: call after rt_stt_finalize");
    if (!p) { s->pr_set = false; s->pr = rt_stt_prompt{}; s->pr_initial.clear(); return RT_OK; }
    const rt_stt_config& c = s->cfg;
    if (s->ts_begin <= 0) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_prompt: the handle has no timestamp ids (rt_stt_set_timestamps)");
    if (p->sot_prev_id <= c.eos_id || p->sot_prev_id >= c.vocab)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_prompt: <|startofprev|> = %d is not a special id of the vocabulary of %d (above end-of-sequence %d)", p->sot_prev_id, c.vocab, c.eos_id);
    if (p->n_initial < 0 || (p->n_initial > 0 && !p->h_initial)) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_prompt: %d initial ids without an array", p->n_initial);
    for (int i = 0; i < p->n_initial; ++i)
        if (p->h_initial[i] < 0 || p->h_initial[i] >= c.vocab) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_prompt: initial id %d outside the vocabulary of %d", p->h_initial[i], c.vocab);
    if (p->reset_on_temperature < 0.f || std::isinf(p->reset_on_temperature)) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_prompt: a reset temperature of %g (>= 0, finite, or NaN for none)", (double)p->reset_on_temperature);
    if (!p->condition_on_previous && p->n_initial == 0) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_prompt: a policy neither conditions on previous text nor carries an initial prompt");
    if (stt_prompt_cap(c) < 1 || stt_max_prefix(c) > c.n_text_ctx - 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_prompt: a text context of %d has no room for a prompt behind %d forced ids", c.n_text_ctx, c.n_prefix);
    s->pr = *p;
    s->pr_initial.assign(p->h_initial, p->h_initial + p->n_initial);
    s->pr.h_initial = nullptr;
    s->pr_set = true;
    return RT_OK;
}

int rt_stt_prompt_report(rt_stt* s, int32_t cap, int32_t* h_prompt_len, int32_t* h_reset, int32_t* n_windows) {
    if (!s || cap < 0 || !n_windows) return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_stt_prompt_report: bad argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    const int32_t n = (int32_t)s->pr_report.size();
    *n_windows = n;
    for (int32_t w = 0; w < std::min(n, cap); ++w) {
        if (h_prompt_len) h_prompt_len[w] = s->pr_report[w].first;
        if (h_reset) h_reset[w] = s->pr_report[w].second;
    }
    if (n > cap) return rt_fail(ctx, RT_ERR_LENGTH, "rt_stt_prompt_report: %d windows, room for %d", n, cap);
    return RT_OK;
}

int rt_stt_fallback_report(rt_stt* s, int32_t cap, int32_t* h_attempts, float* h_temperature, float* h_ratio, int32_t* n_windows) {
    if (!s || cap < 0 || !n_windows) return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_stt_fallback_report: bad argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    const int32_t n = (int32_t)s->fb_report.size();
    *n_windows = n;
    for (int32_t w = 0; w < std::min(n, cap); ++w) {
        if (h_attempts) h_attempts[w] = s->fb_report[w].attempts;
        if (h_temperature) h_temperature[w] = s->fb_report[w].temperature;
        if (h_ratio) h_ratio[w] = s->fb_report[w].ratio;
    }
    if (n > cap) return rt_fail(ctx, RT_ERR_LENGTH, "rt_stt_fallback_report: %d windows, room for %d", n, cap);
    return RT_OK;
}

int rt_debug_stt_probe(rt_stt* s, const float* d_logits, int64_t row_stride, int32_t n_rows, int32_t* h_lang, float* h_lang_prob, float* h_no_speech) {
    if (!s || !d_logits || !h_lang || !h_lang_prob || !h_no_speech || n_rows < 1 || n_rows > STT_GROUP || row_stride < s->cfg.vocab)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_debug_stt_probe: bad argument (1 .. %d rows, row_stride >= vocab)", STT_GROUP);
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_debug_stt_probe: not finalized");
    if (s->lang_ids.empty()) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_stt_probe: the handle has no languages (rt_stt_set_languages)");
    RT_TRY(stt_probe(s, d_logits, row_stride, n_rows));
    s->h_probe.resize(4 * STT_GROUP);
    RT_HIP(ctx, hipMemcpyAsync(s->h_probe.data(), s->d_probe, 3 * STT_GROUP * 4, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const float* pf = (const float*)s->h_probe.data();
    for (int b = 0; b < n_rows; ++b) { h_lang[b] = s->h_probe[b]; h_lang_prob[b] = pf[STT_GROUP + b]; h_no_speech[b] = pf[2 * STT_GROUP + b]; }
    return RT_OK;
}

}  // extern "C"

namespace {
// rt_debug_stt_beam_step, and - ts given - rt_debug_stt_beam_step_ts: the timestamp instantiation with the rows' history state
// (flags, last timestamp) copied in before the step and out behind it
int stt_debug_beam_step(const char* who, rt_stt* s, const float* d_logits, int32_t row_stride, const float* h_scores_in, int32_t n_windows, int32_t beam,
                        const int32_t* h_n_live, const int32_t* h_n_finished, const int32_t* h_done, int32_t first_step, int32_t step,
                        int32_t* h_next_tok, int32_t* h_parent, float* h_scores_out, int32_t* h_n_live_out, int32_t* h_fin_beam, float* h_fin_score,
                        int32_t* h_n_finished_out, int32_t* h_done_out, int32_t* h_live_windows, const SttTsRule* ts = nullptr, const int32_t* h_flags_in = nullptr,
                        const int32_t* h_last_in = nullptr, int32_t* h_flags_out = nullptr, int32_t* h_last_out = nullptr) {
    if (!s || !d_logits || !h_scores_in || !h_n_live || !h_n_finished || !h_done || !h_next_tok || !h_parent || !h_scores_out || !h_n_live_out || !h_fin_beam ||
        !h_fin_score || !h_n_finished_out || !h_done_out || !h_live_windows || beam < 1 || beam > STT_BEAM_MAX || n_windows < 1 ||
        n_windows * beam > STT_GROUP || (row_stride != 1 && row_stride != beam) || step < 0 || step >= s->cfg.max_new_tokens)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "%s: bad argument (windows x beam <= %d, row_stride 1 or beam)", who, STT_GROUP);
    int live = 0;
    for (int w = 0; w < n_windows; ++w) {
        if (h_n_live[w] < 0 || h_n_live[w] > std::min(beam, row_stride) || h_n_finished[w] < 0 || h_n_finished[w] > beam)
            return rt_fail(s->ctx, RT_ERR_INVALID, "%s: window %d: live rows or finished entries out of range", who, w);
        live += h_done[w] ? 0 : 1;
    }
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "%s: not finalized", who);
    const int R = n_windows * beam;
    RT_TRY(stt_beam_reserve(s, R));
    SttBeam& bm = s->beam;
    const SttBeamBook& bk = bm.book;
    std::vector<int32_t>& hb = s->h_book;
    hb.assign(bm.book_n, 0);
    SttBeamBook h = stt_beam_book(hb.data(), bm.rows, s->cfg.max_new_tokens);
    for (int r = 0; r < R; ++r) { h.score[r] = h_scores_in[r]; h.next_tok[r] = -1; h.src[r] = -1; }
    if (ts)
        for (int r = 0; r < R; ++r) { h.ts_flags[r] = h_flags_in[r]; h.ts_last[r] = h_last_in[r]; }
    for (int w = 0; w < n_windows; ++w) { h.n_live[w] = h_n_live[w]; h.n_fin[w] = h_n_finished[w]; h.done[w] = h_done[w] ? 1 : 0; }
    *h.live = live;
    RT_HIP(ctx, hipMemcpyAsync(bm.book_mem, hb.data(), bm.book_n * 4, hipMemcpyHostToDevice, ctx->stream));
    RT_TRY(stt_beam_select(s, d_logits, row_stride, n_windows, first_step ? 1 : 0, beam, step, bk, ts));
    RT_TRY(stt_book_fetch(s, &h));
    for (int r = 0; r < R; ++r) {
        h_next_tok[r] = h.next_tok[r]; h_parent[r] = h.src[r]; h_scores_out[r] = h.score[r];
        h_fin_beam[r] = h.fin_beam[r]; h_fin_score[r] = h.fin_score[r];
    }
    for (int w = 0; w < n_windows; ++w) { h_n_live_out[w] = h.n_live[w]; h_n_finished_out[w] = h.n_fin[w]; h_done_out[w] = h.done[w]; }
    if (ts)
        for (int r = 0; r < R; ++r) { h_flags_out[r] = h.ts_flags[r]; h_last_out[r] = h.ts_last[r]; }
    *h_live_windows = *h.live;
    return RT_OK;
}
}  // namespace

extern "C" {

int rt_debug_stt_beam_step(rt_stt* s, const float* d_logits, int32_t row_stride, const float* h_scores_in, int32_t n_windows, int32_t beam,
                           const int32_t* h_n_live, const int32_t* h_n_finished, const int32_t* h_done, int32_t first_step, int32_t step,
                           int32_t* h_next_tok, int32_t* h_parent, float* h_scores_out, int32_t* h_n_live_out, int32_t* h_fin_beam, float* h_fin_score,
                           int32_t* h_n_finished_out, int32_t* h_done_out, int32_t* h_live_windows) {
    return stt_debug_beam_step("rt_debug_stt_beam_step", s, d_logits, row_stride, h_scores_in, n_windows, beam, h_n_live, h_n_finished, h_done, first_step, step,
                               h_next_tok, h_parent, h_scores_out, h_n_live_out, h_fin_beam, h_fin_score, h_n_finished_out, h_done_out, h_live_windows);
}

int rt_debug_stt_beam_step_ts(rt_stt* s, const float* d_logits, int32_t row_stride, const float* h_scores_in, int32_t n_windows, int32_t beam,
                              const int32_t* h_n_live, const int32_t* h_n_finished, const int32_t* h_done, int32_t first_step, int32_t step,
                              int32_t max_initial_timestamp_index, const int32_t* h_ts_flags_in, const int32_t* h_ts_last_in,
                              int32_t* h_next_tok, int32_t* h_parent, float* h_scores_out, int32_t* h_n_live_out, int32_t* h_fin_beam, float* h_fin_score,
                              int32_t* h_n_finished_out, int32_t* h_done_out, int32_t* h_live_windows, int32_t* h_ts_flags_out, int32_t* h_ts_last_out) {
    if (!s || s->ts_begin <= 0 || !h_ts_flags_in || !h_ts_last_in || !h_ts_flags_out || !h_ts_last_out || max_initial_timestamp_index < -1)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_debug_stt_beam_step_ts: bad argument (a handle with rt_stt_set_timestamps, the rows' history state)");
    const SttTsRule rule{s->ts_begin, s->ts_count, max_initial_timestamp_index};
    return stt_debug_beam_step("rt_debug_stt_beam_step_ts", s, d_logits, row_stride, h_scores_in, n_windows, beam, h_n_live, h_n_finished, h_done, first_step, step,
                               h_next_tok, h_parent, h_scores_out, h_n_live_out, h_fin_beam, h_fin_score, h_n_finished_out, h_done_out, h_live_windows, &rule,
                               h_ts_flags_in, h_ts_last_in, h_ts_flags_out, h_ts_last_out);
}

}  // extern "C"

namespace {
// rt_debug_stt_sample_step, and - ts given - rt_debug_stt_sample_step_ts: k_stt_sample_select over a book of its own (n_rows rows,
// allocated for the call: the handle's decoder side is not grown for a test's row count)
int stt_debug_sample_step(const char* who, rt_stt* s, const float* d_logits, int32_t row_stride, int32_t n_rows, int32_t samples, float temperature, uint64_t seed,
                          int32_t temperature_index, const int32_t* h_key, const int32_t* h_sample, const float* h_scores_in, const int32_t* h_done,
                          int32_t first_step, int32_t step, int32_t* h_next_tok, float* h_scores_out, float* h_win_val, int32_t* h_done_out, int32_t* h_live_rows,
                          const SttTsRule* ts = nullptr, const int32_t* h_flags_in = nullptr, const int32_t* h_last_in = nullptr, int32_t* h_flags_out = nullptr,
                          int32_t* h_last_out = nullptr) {
    if (!s || !d_logits || !h_key || !h_sample || !h_scores_in || !h_done || !h_next_tok || !h_scores_out || !h_win_val || !h_done_out || !h_live_rows ||
        n_rows < 1 || n_rows > 8192 || samples < 1 || samples > STT_BEAM_MAX || n_rows % samples || (row_stride != 1 && row_stride != samples) ||
        !(temperature > 0.f) || std::isinf(temperature) || temperature_index < 0 || step < 0 || step >= s->cfg.max_new_tokens)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "%s: bad argument (1 .. 8192 rows in windows of `samples` 1 .. %d, row_stride 1 or samples, temperature > 0)",
                       who, STT_BEAM_MAX);
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "%s: not finalized", who);
    const int R = n_rows, steps = step + 1;
    const size_t book_n = stt_beam_book_words(R, steps), n = book_n + 3 * (size_t)R;       // book | key | sample | winning value
    std::vector<int32_t> hb(n, 0);
    SttBeamBook h = stt_beam_book(hb.data(), R, steps);
    int live = 0;
    for (int r = 0; r < R; ++r) {
        h.score[r] = h_scores_in[r]; h.next_tok[r] = -1; h.src[r] = -1; h.done[r] = h_done[r] ? 1 : 0;
        hb[book_n + r] = h_key[r]; hb[book_n + R + r] = h_sample[r];
        live += h_done[r] ? 0 : 1;
        if (ts) { h.ts_flags[r] = h_flags_in[r]; h.ts_last[r] = h_last_in[r]; }
    }
    *h.live = live;
    int32_t* d_mem = nullptr;
    RT_HIP(ctx, hipMalloc((void**)&d_mem, n * 4));
    const SttBeamBook bk = stt_beam_book(d_mem, R, steps);
    const SttSampleRule sr{temperature, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), (unsigned)temperature_index, d_mem + book_n, d_mem + book_n + R};
    int rc = hipMemcpyAsync(d_mem, hb.data(), n * 4, hipMemcpyHostToDevice, ctx->stream) == hipSuccess ? RT_OK : RT_ERR_HIP;
    if (rc == RT_OK) rc = stt_sample_select(s, d_logits, row_stride, R, first_step ? 1 : 0, samples, step, bk, ts, sr, (float*)(d_mem + book_n + 2 * (size_t)R));
    if (rc == RT_OK && hipMemcpyAsync(hb.data(), d_mem, n * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = RT_ERR_HIP;
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_mem);
    if (rc != RT_OK) return rc == RT_ERR_HIP ? rt_fail(ctx, RT_ERR_HIP, "%s: a copy failed", who) : rc;
    RT_HIP(ctx, e);
    const float* val = (const float*)(hb.data() + book_n + 2 * (size_t)R);
    for (int r = 0; r < R; ++r) {
        h_next_tok[r] = h.next_tok[r]; h_scores_out[r] = h.score[r]; h_win_val[r] = val[r]; h_done_out[r] = h.done[r];
        if (ts) { h_flags_out[r] = h.ts_flags[r]; h_last_out[r] = h.ts_last[r]; }
    }
    *h_live_rows = *h.live;
    return RT_OK;
}
}  // namespace

extern "C" {

int rt_debug_stt_sample_step(rt_stt* s, const float* d_logits, int32_t row_stride, int32_t n_rows, int32_t samples, float temperature, uint64_t seed,
                             int32_t temperature_index, const int32_t* h_key, const int32_t* h_sample, const float* h_scores_in, const int32_t* h_done,
                             int32_t first_step, int32_t step, int32_t* h_next_tok, float* h_scores_out, float* h_win_val, int32_t* h_done_out, int32_t* h_live_rows) {
    return stt_debug_sample_step("rt_debug_stt_sample_step", s, d_logits, row_stride, n_rows, samples, temperature, seed, temperature_index, h_key, h_sample,
                                 h_scores_in, h_done, first_step, step, h_next_tok, h_scores_out, h_win_val, h_done_out, h_live_rows);
}

int rt_debug_stt_sample_step_ts(rt_stt* s, const float* d_logits, int32_t row_stride, int32_t n_rows, int32_t samples, float temperature, uint64_t seed,
                                int32_t temperature_index, const int32_t* h_key, const int32_t* h_sample, const float* h_scores_in, const int32_t* h_done,
                                int32_t first_step, int32_t step, int32_t max_initial_timestamp_index, const int32_t* h_ts_flags_in, const int32_t* h_ts_last_in,
                                int32_t* h_next_tok, float* h_scores_out, float* h_win_val, int32_t* h_done_out, int32_t* h_live_rows, int32_t* h_ts_flags_out,
                                int32_t* h_ts_last_out) {
    if (!s || s->ts_begin <= 0 || !h_ts_flags_in || !h_ts_last_in || !h_ts_flags_out || !h_ts_last_out || max_initial_timestamp_index < -1)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_debug_stt_sample_step_ts: bad argument (a handle with rt_stt_set_timestamps, the rows' history state)");
    const SttTsRule rule{s->ts_begin, s->ts_count, max_initial_timestamp_index};
    return stt_debug_sample_step("rt_debug_stt_sample_step_ts", s, d_logits, row_stride, n_rows, samples, temperature, seed, temperature_index, h_key, h_sample,
                                 h_scores_in, h_done, first_step, step, h_next_tok, h_scores_out, h_win_val, h_done_out,
                                 h_live_rows, &rule, h_ts_flags_in, h_ts_last_in, h_ts_flags_out, h_ts_last_out);
}

}  // extern "C"

namespace {
// rt_debug_stt_beam_reorder (h_lo null: positions [0, len) of every row) and rt_debug_stt_beam_reorder_range ([h_lo[r], h_hi[r]))
int stt_debug_reorder(const char* who, rt_ctx* ctx, int32_t layers, int32_t rows, int32_t heads, int32_t max_pos, int32_t head_dim, const int32_t* h_src, int32_t len,
                      const int32_t* h_lo, const int32_t* h_hi, uint16_t* h_planes) {
    if (!ctx || !h_src || !h_planes || layers < 1 || rows < 1 || rows > STT_GROUP || heads < 1 || max_pos < 1 || head_dim < 32 || head_dim % 32 || len < 0 ||
        len > max_pos || (h_lo && !h_hi))
        return rt_fail(ctx, RT_ERR_INVALID, "%s: bad argument", who);
    for (int r = 0; r < rows; ++r) {
        if (h_src[r] < 0 || h_src[r] >= rows) return rt_fail(ctx, RT_ERR_INVALID, "%s: src[%d] outside the rows", who, r);
        if (h_lo && (h_lo[r] < 0 || h_hi[r] < h_lo[r] || h_hi[r] > max_pos)) return rt_fail(ctx, RT_ERR_INVALID, "%s: row %d: range [%d, %d) outside [0, %d]", who, r, h_lo[r], h_hi[r], max_pos);
    }
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)layers * rows * heads * max_pos * head_dim;           // one plane
    std::vector<uint16_t> host(8 * n);
    for (int q = 0; q < 4; ++q)
        for (size_t i = 0; i < n; ++i) {
            host[q * n + i] = (uint16_t)((i * 40503u + (size_t)q * 12289u) & 0x7fffu);       // the source cache: a value per (plane, layer, row, head, pos, dim)
            host[(4 + q) * n + i] = 0xbeef;                                                 // the destination: a sentinel
        }
    bf16_t* d = nullptr;
    int32_t* d_src = nullptr;                              // src | lo | hi
    RT_HIP(ctx, hipMalloc((void**)&d, 8 * n * 2));
    auto run = [&]() -> int {
        RT_HIP(ctx, hipMalloc((void**)&d_src, (size_t)rows * 3 * 4));
        RT_HIP(ctx, hipMemcpyAsync(d, host.data(), 8 * n * 2, hipMemcpyHostToDevice, ctx->stream));
        RT_HIP(ctx, hipMemcpyAsync(d_src, h_src, (size_t)rows * 4, hipMemcpyHostToDevice, ctx->stream));
        if (h_lo) {
            RT_HIP(ctx, hipMemcpyAsync(d_src + rows, h_lo, (size_t)rows * 4, hipMemcpyHostToDevice, ctx->stream));
            RT_HIP(ctx, hipMemcpyAsync(d_src + 2 * rows, h_hi, (size_t)rows * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        KvCache a, b;
        a.layers = b.layers = layers; a.slots = b.slots = rows; a.kv_heads = b.kv_heads = heads; a.max_pos = b.max_pos = max_pos; a.head_dim = b.head_dim = head_dim;
        a.k = d; a.v = d + n; a.k_lo = d + 2 * n; a.v_lo = d + 3 * n;
        b.k = d + 4 * n; b.v = d + 5 * n; b.k_lo = d + 6 * n; b.v_lo = d + 7 * n;
        if (h_lo) RT_TRY(stt_beam_reorder_range(ctx, a, b, d_src, d_src + rows, d_src + 2 * rows, rows));
        else RT_TRY(stt_beam_reorder(ctx, a, b, d_src, rows, len));
        RT_HIP(ctx, hipMemcpyAsync(h_planes, d, 8 * n * 2, hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return RT_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d);
    if (d_src) (void)hipFree(d_src);
    return rc;
}
}  // namespace

extern "C" {

int rt_debug_stt_beam_reorder(rt_ctx* ctx, int32_t layers, int32_t rows, int32_t heads, int32_t max_pos, int32_t head_dim, const int32_t* h_src, int32_t len,
                              uint16_t* h_planes) {
    return stt_debug_reorder("rt_debug_stt_beam_reorder", ctx, layers, rows, heads, max_pos, head_dim, h_src, len, nullptr, nullptr, h_planes);
}

int rt_debug_stt_beam_reorder_range(rt_ctx* ctx, int32_t layers, int32_t rows, int32_t heads, int32_t max_pos, int32_t head_dim, const int32_t* h_src,
                                    const int32_t* h_lo, const int32_t* h_hi, uint16_t* h_planes) {
    if (!h_lo || !h_hi) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_stt_beam_reorder_range: null range");
    return stt_debug_reorder("rt_debug_stt_beam_reorder_range", ctx, layers, rows, heads, max_pos, head_dim, h_src, 0, h_lo, h_hi, h_planes);
}

int rt_bench_stt_gather(rt_ctx* ctx, int32_t layers, int32_t rows, int32_t heads, int32_t max_pos, int32_t head_dim, int32_t prefix, int32_t step, int32_t iters,
                        double* us_ranged, double* us_uniform) {
    if (!ctx || !us_ranged || !us_uniform || layers < 1 || rows < 1 || rows > STT_GROUP || heads < 1 || max_pos < 1 || head_dim < 32 || head_dim % 32 || prefix < 0 ||
        step < 0 || prefix + step > max_pos || iters < 1)
        return rt_fail(ctx, RT_ERR_INVALID, "rt_bench_stt_gather: bad argument (rows <= %d, prefix + step <= max_pos)", STT_GROUP);
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)layers * rows * heads * max_pos * head_dim;           // one plane
    std::vector<int32_t> tab(3 * (size_t)rows);                                    // src (neighbours swap) | lo | hi
    for (int r = 0; r < rows; ++r) { tab[r] = (r ^ 1) < rows ? (r ^ 1) : r; tab[rows + r] = prefix; tab[2 * rows + r] = prefix + step; }
    bf16_t* d = nullptr;
    int32_t* d_tab = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        RT_HIP(ctx, hipMalloc((void**)&d, 8 * n * 2));
        RT_HIP(ctx, hipMalloc((void**)&d_tab, tab.size() * 4));
        RT_HIP(ctx, hipMemsetAsync(d, 0, 8 * n * 2, ctx->stream));
        RT_HIP(ctx, hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        RT_HIP(ctx, hipEventCreate(&e0)); RT_HIP(ctx, hipEventCreate(&e1));
        KvCache a, b;
        a.layers = b.layers = layers; a.slots = b.slots = rows; a.kv_heads = b.kv_heads = heads; a.max_pos = b.max_pos = max_pos; a.head_dim = b.head_dim = head_dim;
        a.k = d; a.v = d + n; a.k_lo = d + 2 * n; a.v_lo = d + 3 * n;
        b.k = d + 4 * n; b.v = d + 5 * n; b.k_lo = d + 6 * n; b.v_lo = d + 7 * n;
        for (int form = 0; form < 2; ++form) {
            float ms = 0.f;
            for (int i = -1; i < iters; ++i) {                 // (one launch before the clock starts)
                if (i == 0) RT_HIP(ctx, hipEventRecord(e0, ctx->stream));
                if (form == 0) RT_TRY(stt_beam_reorder_range(ctx, i & 1 ? b : a, i & 1 ? a : b, d_tab, d_tab + rows, d_tab + 2 * rows, rows));
                else RT_TRY(stt_beam_reorder(ctx, i & 1 ? b : a, i & 1 ? a : b, d_tab, rows, prefix + step));
            }
            RT_HIP(ctx, hipEventRecord(e1, ctx->stream));
            RT_HIP(ctx, hipEventSynchronize(e1));
            RT_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
            *(form == 0 ? us_ranged : us_uniform) = (double)ms * 1e3 / iters;
        }
        return RT_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(ctx->stream);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d) (void)hipFree(d);
    if (d_tab) (void)hipFree(d_tab);
    return rc;
}

int rt_debug_stt_prompt_prefix(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_windows, int32_t sample_rate, const int32_t* h_tokens,
                               const int32_t* h_len, float* d_logits) {
    if (!s || !h_tokens || !h_len || !d_logits || n_windows < 1 || n_windows > STT_GROUP || sample_rate < 1000 || stt_check_clips(d_pcm, n_samples, n_windows))
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_debug_stt_prompt_prefix: bad argument (1 .. %d windows)", STT_GROUP);
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_debug_stt_prompt_prefix: not finalized");
    const rt_stt_config& c = s->cfg;
    std::vector<std::vector<int32_t>> toks(n_windows);
    for (int w = 0, at = 0; w < n_windows; ++w) {
        if (h_len[w] < 1 || h_len[w] > std::min(stt_max_prefix(c), c.n_text_ctx - 1))
            return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_stt_prompt_prefix: window %d: %d tokens (1 .. %d)", w, h_len[w], std::min(stt_max_prefix(c), c.n_text_ctx - 1));
        for (int i = 0; i < h_len[w]; ++i, ++at) {
            if (h_tokens[at] < 0 || h_tokens[at] >= c.vocab) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_stt_prompt_prefix: token %d outside the vocabulary of %d", h_tokens[at], c.vocab);
            toks[w].push_back(h_tokens[at]);
        }
    }
    std::vector<SttSpan> group;
    stt_cut(c, sample_rate, d_pcm, n_samples, n_windows, group, true);
    RT_TRY(stt_group_reserve(s, n_windows));
    RT_TRY(stt_beam_reserve(s, n_windows));
    RT_TRY(stt_prompt_reserve(s, n_windows, n_windows));
    RT_TRY(stt_prompt_tables(s, toks, nullptr, n_windows, 1));
    RT_TRY(stt_features_group(s, group.data(), n_windows, sample_rate));
    RT_TRY(stt_encode(s, s->grp.enc, n_windows));
    RT_TRY(stt_prompt_prefix_pass(s, s->beam.dec.kv, s->beam.dec.logits, false, 0));
    RT_HIP(ctx, hipMemcpyAsync(d_logits, s->beam.dec.logits, (size_t)n_windows * c.vocab * 4, hipMemcpyDeviceToDevice, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_debug_stt_encode_batch(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips, int32_t sample_rate, float* d_states) {
    if (!s || !d_states || n_clips < 1 || n_clips > STT_GROUP || sample_rate < 1000 || stt_check_clips(d_pcm, n_samples, n_clips))
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_debug_stt_encode_batch: bad argument (1 .. %d clips)", STT_GROUP);
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_debug_stt_encode_batch: not finalized");
    std::vector<SttSpan> group;
    stt_cut(s->cfg, sample_rate, d_pcm, n_samples, n_clips, group, true);
    RT_TRY(stt_group_reserve(s, n_clips));
    RT_TRY(stt_features_group(s, group.data(), n_clips, sample_rate));
    RT_TRY(stt_encode(s, s->grp.enc, n_clips));
    RT_HIP(ctx, hipMemcpyAsync(d_states, s->grp.enc.out, (size_t)n_clips * s->cfg.n_ctx * s->cfg.d_model * 4, hipMemcpyDeviceToDevice, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

}  // extern "C"

extern "C" {

int rt_stt_set_alignment(rt_stt* s, const int32_t* h_layer_head, int32_t n_heads, int32_t median_width) {
    if (!s || !h_layer_head) return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_stt_set_alignment: null argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    const rt_stt_config& c = s->cfg;
    if (n_heads < 1 || n_heads > ALIGN_HEADS_MAX) return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_alignment: %d heads (1 .. %d)", n_heads, ALIGN_HEADS_MAX);
    if (median_width < 1 || median_width > ALIGN_MEDIAN_MAX || !(median_width & 1))
        return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_alignment: a median width of %d (odd, 1 .. %d)", median_width, ALIGN_MEDIAN_MAX);
    std::vector<std::pair<int32_t, int32_t>> heads;
    std::vector<AlignHeads> layers(c.dec_layers, AlignHeads{});
    for (int i = 0; i < n_heads; ++i) {
        const int32_t l = h_layer_head[2 * i], h = h_layer_head[2 * i + 1];
        if (l < 0 || l >= c.dec_layers || h < 0 || h >= c.heads)
            return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_alignment: pair %d = (%d, %d) outside %d decoder layers of %d heads", i, l, h, c.dec_layers, c.heads);
        if (std::find(heads.begin(), heads.end(), std::make_pair(l, h)) != heads.end())
            return rt_fail(ctx, RT_ERR_INVALID, "rt_stt_set_alignment: pair (%d, %d) is given twice", l, h);
        heads.push_back({l, h});
        AlignHeads& a = layers[l];
        a.head[a.n] = h; a.out[a.n] = i; ++a.n;
    }
    s->al_heads = std::move(heads);
    s->al_layers = std::move(layers);
    s->al_width = median_width;
    return RT_OK;
}

int rt_stt_align(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_windows, int32_t sample_rate, const int32_t* h_text_ids,
                 const int32_t* h_text_offsets, const int32_t* h_language, rt_stt_align_out* out) {
    if (!s || !out) return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_stt_align: null argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<SttAlignItem> items;
    RT_TRY(stt_align_check(s, "rt_stt_align", d_pcm, n_samples, n_windows, sample_rate, h_text_ids, h_text_offsets, h_language, items));
    if (out->h_n_frames)
        for (int w = 0; w < n_windows; ++w) out->h_n_frames[w] = stt_align_frames(s->cfg, sample_rate, n_samples[w]);
    // groups of up to STT_GROUP windows with ids, in the call's order; a window without ids has no entries and takes part in nothing
    std::vector<SttAlignItem> group;
    size_t f_at = 0, l_at = 0;
    for (size_t next = 0; next <= items.size(); ++next) {
        if (next < items.size() && items[next].n > 0) group.push_back(items[next]);
        if (group.empty() || (next < items.size() && (int)group.size() < STT_GROUP)) continue;
        size_t A = 0, L = 0;
        for (const SttAlignItem& it : group) { A += (size_t)it.n + 1; L += it.n; }
        RT_TRY(stt_align_group(s, group.data(), (int)group.size(), sample_rate, out->h_token_frame ? out->h_token_frame + f_at : nullptr,
                               out->h_token_logprob ? out->h_token_logprob + l_at : nullptr, nullptr));
        f_at += A; l_at += L;
        group.clear();
    }
    return RT_OK;
}

int rt_debug_stt_align_timing(rt_stt* s, int32_t on, double* ms_capture, double* ms_matrix, double* ms_dtw) {
    if (!s) return RT_ERR_INVALID;
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    if (ms_capture) *ms_capture = s->al_ms[0];
    if (ms_matrix) *ms_matrix = s->al_ms[1];
    if (ms_dtw) *ms_dtw = s->al_ms[2];
    for (double& v : s->al_ms) v = 0.0;
    s->al_clock = on != 0;
    return RT_OK;
}

int rt_debug_stt_align_stages(rt_stt* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_windows, int32_t sample_rate, const int32_t* h_text_ids,
                              const int32_t* h_text_offsets, const int32_t* h_language, float* h_W, int64_t w_cap, float* h_M, int64_t m_cap, int32_t* h_shape,
                              int32_t* h_token_frame, float* h_token_logprob) {
    if (!s || !h_W || !h_M || !h_shape || w_cap < 0 || m_cap < 0 || n_windows < 1 || n_windows > STT_GROUP)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_debug_stt_align_stages: bad argument (1 .. %d windows)", STT_GROUP);
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<SttAlignItem> items;
    RT_TRY(stt_align_check(s, "rt_debug_stt_align_stages", d_pcm, n_samples, n_windows, sample_rate, h_text_ids, h_text_offsets, h_language, items));
    for (const SttAlignItem& it : items)
        if (it.n < 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_stt_align_stages: every window needs text ids");
    SttAlignStages st{h_W, (size_t)w_cap, h_M, (size_t)m_cap, 0, 0};
    const int rc = stt_align_group(s, items.data(), n_windows, sample_rate, h_token_frame, h_token_logprob, &st);
    h_shape[0] = st.r_max; h_shape[1] = st.f_max;
    return rc;
}

}  // extern "C"
