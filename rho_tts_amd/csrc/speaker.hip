// The GE2E speaker encoder (resemblyzer's VoiceEncoder) on a waveform that already lives in HBM: the first 256 dimensions of the
// drift classifier's 286-d vector (validation/classifier/trainer.py:23-68) and the space of
// _compute_speaker_similarity (base_tts.py:325-346).
//
//   PCM at the TTS rate -> windowed-sinc resampler (16 kHz; resample.h, the resampler of the STT and feature front ends)
//     -> normalize_volume(-30 dBFS, increase_only): rms over the whole clip in float64; a quieter clip is scaled up, a clip of
//        zeros is left alone (DEVIATION: resemblyzer divides by zero there)
//     -> trim_long_silences, ONLY when the caller supplies voice flags (one per 480-sample window; resemblyzer's come from webrtcvad,
//        which is neither restated nor replaced here): moving average of 8, round half to even, dilation by 7 - integer work on a
//        few hundred flags that the host does, because the kept length decides every later grid - and a compaction of the kept
//        windows on the device.  Without flags nothing is cut (DEVIATION, the default)
//     -> partial slices (rate 1.3, coverage 0.75: 160 mel frames every 77), zero padding up to the last partial's end
//     -> mel: frames of 400 (hop 160, zero-padded centre), periodic Hann, 400-point DFT in float64, POWER spectrum, 40 slaney
//        filters 0 .. 8 kHz, no log, float32
//     -> gather of the partials [P][160][40]
//     -> 3 x LSTM-256 (torch.nn.LSTM: gates i, f, g, o, two biases, zero initial state): k_spk_lstm, one launch per layer
//     -> per partial relu(W h_T + b) / norm; per clip mean of its partials / norm (a zero norm gives zeros, not NaN)
//
// As in features.hip a small device table (SpkClip) tells every kernel where a clip's samples, frames and partials are, every stage
// is one launch for the call (the recurrent stage one per layer), no front-end launch mixes clips, and the handle holds one
// workspace set, grown on demand.  The recurrent kernel tiles PARTIALS, 16 to a workgroup, from whichever clips they come: every
// row of a tile is its own k-ordered chain of f32 fmas (below), so a partial's bits depend neither on its row nor on its neighbours.
//
// PARITY UNPINNED (resemblyzer, webrtcvad and librosa are absent; no pretrained weights offline): the definition is
// resemblyzer 0.1.x restated, and tests/speaker_embed_ref.py is its float64 oracle.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "kernels.h"
#include "resample.h"

struct SpkClip {
    const float* pcm_in;    // the clip's samples at the input rate
    const float* pcm16;     // ... at 16 kHz: its stretch of the resampler's output, or pcm_in itself when the rates agree
    float* pre;             // ... preprocessed (scaled, compacted), n_pad floats, zeros behind n_pre
    const int* win_dst;     // [n_win]: the window's place among the kept ones, -1 = dropped; null = no voice flags, nothing is cut
    int64_t n_in, n16, n_pre, n_pad;
    int32_t n_win;
    int32_t first_frame, frames;      // in the frame-major mel workspace of the call
    int32_t first_part, parts;        // in the partial-major workspaces of the call
};

template <class T>
struct SpkBuf { T* p = nullptr; size_t cap = 0; };

constexpr int S_SR = 16000, S_NFFT = 400, S_HOP = 160, S_BINS = S_NFFT / 2 + 1, S_MELS = 40;
constexpr int S_H = 256, S_G = 4 * S_H, S_T = 160, S_STEP = 77, S_LAYERS = 3, S_TILE = 16, S_WIN = 480;
constexpr int S_KIN0 = 64;                         // layer 0's 40 inputs, zero-padded: an even count of k groups of 16 (48 makes 19, and the k loop spills)
constexpr int S_MAX_PARTS = 4096;                  // per call: two [P][160][256] float32 sequences, 1.3 GB at the cap

struct rt_spk {
    rt_ctx* ctx = nullptr;
    bool finalized = false;
    // host copies of the tensors (torch's names) until rt_spk_finalize packs and uploads them
    std::vector<float> w_ih[S_LAYERS], w_hh[S_LAYERS], b_ih[S_LAYERS], b_hh[S_LAYERS], lin_w, lin_b, melf, win;
    float* d_wp[S_LAYERS] = {nullptr, nullptr, nullptr};   // [16 hidden tiles][4 gates][k groups][64 lanes][4]: the B fragments of k_spk_lstm
    float* d_bias[S_LAYERS] = {nullptr, nullptr, nullptr}; // [1024] = bias_ih + bias_hh (float32 sum)
    float *d_lin_w = nullptr, *d_lin_b = nullptr;          // [256][256], [256]
    float* d_melT = nullptr;                               // [201][40]
    double *d_win = nullptr, *d_twc = nullptr, *d_tws = nullptr;   // window [400], cos / sin(2 pi n / 400)
    Resampler rs;
    SpkBuf<float> pcm, pre, mel, parts, seq_a, seq_b, h_last, pemb, emb;
    SpkBuf<double> scale;                          // [clips]
    SpkBuf<int> win_dst, part_row;                 // every clip's window table back to back; [P] first mel row of a partial
    SpkBuf<SpkClip> clips;
    std::vector<SpkClip> h_clips;
    std::vector<int> h_win_dst, h_part_row;
};

namespace {

__global__ void k_spk_resample(const SpkClip* __restrict__ clips, int L, int M, int taps, int half, const float* __restrict__ h) {
    const SpkClip c = clips[blockIdx.y];
    float* y = const_cast<float*>(c.pcm16);
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < c.n16; n += (int64_t)gridDim.x * blockDim.x)
        y[n] = resample_at(c.pcm_in, c.n_in, n, L, M, taps, half, h);
}

// scale[clip] of normalize_volume: one workgroup per clip, float64 sum of squares (strided per thread, then a fixed tree)
__global__ __launch_bounds__(1024) void k_spk_rms(const SpkClip* __restrict__ clips, double* __restrict__ scale) {
    __shared__ double sh[1024];
    const SpkClip c = clips[blockIdx.x];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t n = tid; n < c.n16; n += 1024) { const double v = (double)c.pcm16[n]; s += v * v; }
    sh[tid] = s;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        const double rms = sqrt(sh[0] / (double)c.n16);
        double g = 1.0;
        if (rms > 0.0) {
            const double change = -30.0 - 20.0 * log10(rms);
            if (change > 0.0) g = pow(10.0, change / 20.0);
        }
        scale[blockIdx.x] = g;
    }
}

// pre = the scaled clip, with voice flags only its kept windows, moved up (a window's destination comes from the host's table)
__global__ void k_spk_scale_compact(const SpkClip* __restrict__ clips, const double* __restrict__ scale) {
    const SpkClip c = clips[blockIdx.y];
    const double g = scale[blockIdx.y];
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < c.n16; n += (int64_t)gridDim.x * blockDim.x) {
        int64_t dst = n;
        if (c.win_dst) {
            const int64_t w = n / S_WIN;
            if (w >= c.n_win) continue;                   // the clip is cut to a multiple of 480
            const int d = c.win_dst[w];
            if (d < 0) continue;
            dst = (int64_t)d * S_WIN + (n - w * S_WIN);
        }
        if (dst < c.n_pad) c.pre[dst] = (float)((double)c.pcm16[n] * g);
    }
}

// One mel frame per workgroup: frame f covers samples [160 f - 200, 160 f + 200) of the padded clip (zeros outside), times the window;
// bin k on thread k: direct DFT with the twiddle index k n mod 400; then the 40 filters on threads 0 .. 39.
__global__ __launch_bounds__(256) void k_spk_mel(const SpkClip* __restrict__ clips, const double* __restrict__ win, const double* __restrict__ twc,
                                                 const double* __restrict__ tws, const float* __restrict__ melT, float* __restrict__ mel) {
    __shared__ double xw[S_NFFT], tc[S_NFFT], ts[S_NFFT], pw[S_BINS];
    const SpkClip clip = clips[blockIdx.y];
    if ((int)blockIdx.x >= clip.frames) return;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int64_t start = (int64_t)f * S_HOP - S_NFFT / 2;
    for (int i = tid; i < S_NFFT; i += 256) {
        const int64_t t = start + i;
        const double v = (t >= 0 && t < clip.n_pad) ? (double)clip.pre[t] : 0.0;
        tc[i] = twc[i];
        ts[i] = tws[i];
        xw[i] = v * win[i];
    }
    __syncthreads();
    if (tid < S_BINS) {
        double re = 0.0, im = 0.0;
        int idx = 0;
        for (int i = 0; i < S_NFFT; ++i) {
            re += xw[i] * tc[idx];
            im -= xw[i] * ts[idx];
            idx += tid;
            if (idx >= S_NFFT) idx -= S_NFFT;
        }
        pw[tid] = re * re + im * im;
    }
    __syncthreads();
    if (tid < S_MELS) {
        double acc = 0.0;
        for (int k = 0; k < S_BINS; ++k) acc += (double)melT[k * S_MELS + tid] * pw[k];
        mel[((int64_t)clip.first_frame + f) * S_MELS + tid] = (float)acc;
    }
}

// parts[p][t][m] = mel[part_row[p] + t][m]
__global__ __launch_bounds__(256) void k_spk_gather(const int* __restrict__ part_row, const float* __restrict__ mel, float* __restrict__ parts) {
    const int p = blockIdx.x;
    const float* src = mel + (int64_t)part_row[p] * S_MELS;
    float* dst = parts + (int64_t)p * S_T * S_MELS;
    for (int i = threadIdx.x; i < S_T * S_MELS; i += 256) dst[i] = src[i];
}

typedef float spk_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float spk_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// One LSTM layer over all 160 steps for a tile of 16 sequences: THE hot path.
//   gates[16][1024] = bias + [x_t | h_{t-1}] . [W_ih | W_hh]^T per step, on __builtin_amdgcn_mfma_f32_16x16x4f32: f32 in, f32
//   accumulate, every gate value one k-ordered chain of f32 fmas - so the result is a property of the sequence alone (any row of any
//   tile gives the same bits) and the error against float64 is that of torch's own float32 LSTM.  bf16 hi + lo planes, the project's
//   other near-f32 idiom, would be about five times the MFMA rate at three products per term; at 1.4 M parameters and a handful of
//   tiles per chunk the kernel is bound by the 160 dependent steps, not by a rate worth trading the exact chain for.
//   The input half is folded into the step (one k loop over KT = KIN + 256): no [P][160][1024] pre-activation workspace, one kernel.
// [x_t | h_{t-1}] lives in LDS (a[16][KT + 4]), c in registers, the weights stream from L2 every step as ready-made B fragments
// (rt_spk_finalize packs them: wave w owns hidden tiles 2 w and 2 w + 1, all four gates of each, so a lane holds i, f, g, o of the
// same (sequence, hidden unit) and updates its c without any exchange).  k group kg covers k = 16 kg .. 16 kg + 15, lane l holds
// k = 16 kg + 4 (l >> 4) + j for the four MFMAs j of the group, on both operands.
// No workgroup waits for another: a sequence's 1024 gate columns are all here.  Rows past n_seq compute on zeros and store nothing.
template <int KIN>      // the layer's input width, zero-padded: 64 (40 mels) or 256
__global__ __launch_bounds__(512) void k_spk_lstm(const float* __restrict__ x, int kin, int n_seq, const spk_f4* __restrict__ wp,
                                                  const float* __restrict__ bias, float* __restrict__ seq_out, float* __restrict__ h_last) {
    constexpr int KT = KIN + S_H, NKG = KT / 16, LD = KT + 4, XN = (S_TILE * KIN + 511) / 512;
    __shared__ __attribute__((aligned(16))) float a[S_TILE * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = blockIdx.x * S_TILE;
    const int col = lane & 15, quad = lane >> 4;
    float c[2][4], b[2][4];
    for (int hh = 0; hh < 2; ++hh)
        for (int g = 0; g < 4; ++g) b[hh][g] = bias[g * S_H + (2 * wave + hh) * 16 + col];
    for (int hh = 0; hh < 2; ++hh)
        for (int r = 0; r < 4; ++r) c[hh][r] = 0.0f;
    for (int i = tid; i < S_TILE * LD; i += 512) a[i] = 0.0f;
    // x of step t for this thread's XN places of the tile (row = place / KIN, k = place % KIN)
    float xn[XN];
    auto load_x = [&](int t) {
#pragma unroll
        for (int q = 0; q < XN; ++q) {
            const int i = tid + q * 512, row = i / KIN, k = i - row * KIN;
            xn[q] = (i < S_TILE * KIN && p0 + row < n_seq && k < kin) ? x[((int64_t)(p0 + row) * S_T + t) * kin + k] : 0.0f;
        }
    };
    auto store_x = [&]() {
#pragma unroll
        for (int q = 0; q < XN; ++q) {
            const int i = tid + q * 512, row = i / KIN, k = i - row * KIN;
            if (i < S_TILE * KIN) a[row * LD + k] = xn[q];
        }
    };
    load_x(0);
    __syncthreads();
    store_x();
    const spk_f4* wbase = wp + (int64_t)(2 * wave) * 4 * NKG * 64 + lane;
    for (int t = 0; t < S_T; ++t) {
        __syncthreads();                            // a = [x_t | h_{t-1}] is complete
        if (t + 1 < S_T) load_x(t + 1);             // (in flight behind the k loop)
        spk_f4 acc[2][4];
        for (int hh = 0; hh < 2; ++hh)
            for (int g = 0; g < 4; ++g) acc[hh][g] = spk_f4{b[hh][g], b[hh][g], b[hh][g], b[hh][g]};
        // (Measured: holding the B fragments of group kg + 1 in a second register set while group kg multiplies changes nothing -
        // 7.65 against 7.35 ms per 256-wide layer - so the loop stays in its plain form; profiles/r14_speaker_embed.txt.)
#pragma unroll 2
        for (int kg = 0; kg < NKG; ++kg) {
            const spk_f4 av = *reinterpret_cast<const spk_f4*>(&a[col * LD + kg * 16 + quad * 4]);
            spk_f4 bv[2][4];
#pragma unroll
            for (int hh = 0; hh < 2; ++hh)
#pragma unroll
                for (int g = 0; g < 4; ++g) bv[hh][g] = wbase[((int64_t)(hh * 4 + g) * NKG + kg) * 64];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh)
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[hh][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[hh][g][j], acc[hh][g], 0, 0, 0);
        }
        __syncthreads();                            // every wave has read a
        // acc[hh][g][r]: sequence row 4 quad + r, hidden unit 16 (2 wave + hh) + col
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int unit = (2 * wave + hh) * 16 + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = quad * 4 + r;
                const float ig = spk_sigmoid(acc[hh][0][r]), fg = spk_sigmoid(acc[hh][1][r]), gg = tanhf(acc[hh][2][r]), og = spk_sigmoid(acc[hh][3][r]);
                c[hh][r] = fg * c[hh][r] + ig * gg;
                const float h = og * tanhf(c[hh][r]);
                a[row * LD + KIN + unit] = h;
                if (p0 + row < n_seq) {
                    if (seq_out) seq_out[((int64_t)(p0 + row) * S_T + t) * S_H + unit] = h;
                    if (h_last && t == S_T - 1) h_last[(int64_t)(p0 + row) * S_H + unit] = h;
                }
            }
        }
        if (t + 1 < S_T) store_x();
    }
}

// sum of v over the 256 threads of the workgroup in a fixed tree, on every thread
__device__ __forceinline__ double spk_block_sum(double v, double* sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    return sh[0];
}

// pemb[p] = e / |e|, e = relu(W h_last[p] + b); one workgroup per partial, unit j on thread j, float64 sums in index order
__global__ __launch_bounds__(256) void k_spk_head(const float* __restrict__ h_last, const float* __restrict__ w, const float* __restrict__ b,
                                                  float* __restrict__ pemb) {
    __shared__ double sh[256];
    __shared__ float hv[S_H];
    const int p = blockIdx.x, j = threadIdx.x;
    hv[j] = h_last[(int64_t)p * S_H + j];
    __syncthreads();
    double acc = (double)b[j];
    for (int k = 0; k < S_H; ++k) acc += (double)w[j * S_H + k] * (double)hv[k];
    const double e = acc > 0.0 ? acc : 0.0;
    const double norm = sqrt(spk_block_sum(e * e, sh));
    pemb[(int64_t)p * S_H + j] = norm > 0.0 ? (float)(e / norm) : 0.0f;
}

// emb[clip] = m / |m|, m = mean of the clip's partial embeddings (in partial order); zeros when |m| = 0
__global__ __launch_bounds__(256) void k_spk_utter(const SpkClip* __restrict__ clips, const float* __restrict__ pemb, float* __restrict__ emb) {
    __shared__ double sh[256];
    const SpkClip c = clips[blockIdx.x];
    const int j = threadIdx.x;
    double s = 0.0;
    for (int i = 0; i < c.parts; ++i) s += (double)pemb[(int64_t)(c.first_part + i) * S_H + j];
    const double m = s / (double)c.parts;
    const double norm = sqrt(spk_block_sum(m * m, sh));
    emb[(int64_t)blockIdx.x * S_H + j] = norm > 0.0 ? (float)(m / norm) : 0.0f;
}

template <class T>
int spk_grow(rt_ctx* ctx, SpkBuf<T>& b, size_t need) {
    if (need <= b.cap && b.p) return RT_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
    if (need == 0) need = 1;
    RT_HIP(ctx, hipMalloc((void**)&b.p, need * sizeof(T)));
    b.cap = need;
    return RT_OK;
}

// compute_partial_slices(n, rate 1.3, min_coverage 0.75): the number of partials and the length the clip is zero-padded to
void spk_partials(int64_t n, int* parts, int64_t* n_pad) {
    const int64_t n_frames = (n + 1 + S_HOP - 1) / S_HOP;
    const int64_t steps = std::max<int64_t>(1, n_frames - S_T + S_STEP + 1);
    int64_t k = (steps + S_STEP - 1) / S_STEP;                  // starts 0, 77, ... below steps
    if (k > 1) {
        const int64_t start_last = (k - 1) * S_STEP;
        // (n - 160 start) / 25600 < 0.75  <=>  n - 160 start < 19200 (exact in integers)
        if (n - S_HOP * start_last < (int64_t)(S_T * S_HOP) * 3 / 4) --k;
    }
    *parts = (int)k;
    *n_pad = std::max<int64_t>(n, S_HOP * ((k - 1) * S_STEP + S_T));
}

// trim_long_silences behind the VAD: flags [n_win] (0 / 1) -> dst [n_win] (place among the kept windows, -1 = dropped); returns the kept count
int spk_smooth_flags(const uint8_t* flags, int n_win, int* dst) {
    std::vector<int> avg2(n_win), mask(n_win);                  // avg2 = 8 x the moving average over [w - 4, w + 3] (3 + 4 zeros of padding, cumsum difference)
    // padded = 3 zeros | flags | 4 zeros; ret[i] = cumsum[i + 7] - cumsum[i - 1] over padded = flags[i - 3 .. i + 4]
    for (int w = 0; w < n_win; ++w) {
        int s = 0;
        for (int o = -3; o <= 4; ++o) { const int q = w + o; if (q >= 0 && q < n_win) s += flags[q] ? 1 : 0; }
        avg2[w] = s;
    }
    for (int w = 0; w < n_win; ++w) mask[w] = avg2[w] > 4 ? 1 : 0;      // round half to even: 4 / 8 = 0.5 -> 0
    int kept = 0;
    for (int w = 0; w < n_win; ++w) {                           // dilation by ones(7): any mask within +-3
        int on = 0;
        for (int o = -3; o <= 3; ++o) { const int q = w + o; if (q >= 0 && q < n_win && mask[q]) on = 1; }
        dst[w] = on ? kept++ : -1;
    }
    return kept;
}

std::vector<float>* spk_slot(rt_spk* s, const std::string& name, int64_t* rows, int64_t* cols) {
    for (int l = 0; l < S_LAYERS; ++l) {
        const std::string sfx = "_l" + std::to_string(l);
        const int64_t kin = l == 0 ? S_MELS : S_H;
        if (name == "lstm.weight_ih" + sfx) { *rows = S_G; *cols = kin; return &s->w_ih[l]; }
        if (name == "lstm.weight_hh" + sfx) { *rows = S_G; *cols = S_H; return &s->w_hh[l]; }
        if (name == "lstm.bias_ih" + sfx) { *rows = S_G; *cols = 1; return &s->b_ih[l]; }
        if (name == "lstm.bias_hh" + sfx) { *rows = S_G; *cols = 1; return &s->b_hh[l]; }
    }
    if (name == "linear.weight") { *rows = S_H; *cols = S_H; return &s->lin_w; }
    if (name == "linear.bias") { *rows = S_H; *cols = 1; return &s->lin_b; }
    if (name == "mel.filters") { *rows = S_BINS; *cols = S_MELS; return &s->melf; }
    if (name == "mel.window") { *rows = S_NFFT; *cols = 1; return &s->win; }
    return nullptr;
}

template <class T>
int spk_upload(rt_ctx* ctx, T** d, const std::vector<T>& h) {
    if (*d) (void)hipFree(*d);
    *d = nullptr;
    RT_HIP(ctx, hipMalloc((void**)d, h.size() * sizeof(T)));
    RT_HIP(ctx, hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return RT_OK;
}

// the three recurrent launches and the per-partial head over parts [P][160][40] (s->parts): leaves pemb [P][256]
int spk_network(rt_spk* s, int P) {
    rt_ctx* ctx = s->ctx;
    RT_TRY(spk_grow(ctx, s->seq_a, (size_t)P * S_T * S_H));
    RT_TRY(spk_grow(ctx, s->seq_b, (size_t)P * S_T * S_H));
    RT_TRY(spk_grow(ctx, s->h_last, (size_t)P * S_H));
    RT_TRY(spk_grow(ctx, s->pemb, (size_t)P * S_H));
    const dim3 tiles((unsigned)((P + S_TILE - 1) / S_TILE));
    hipLaunchKernelGGL(k_spk_lstm<S_KIN0>, tiles, dim3(512), 0, ctx->stream, s->parts.p, S_MELS, P, (const spk_f4*)s->d_wp[0], s->d_bias[0], s->seq_a.p,
                       (float*)nullptr);
    hipLaunchKernelGGL(k_spk_lstm<S_H>, tiles, dim3(512), 0, ctx->stream, s->seq_a.p, S_H, P, (const spk_f4*)s->d_wp[1], s->d_bias[1], s->seq_b.p,
                       (float*)nullptr);
    hipLaunchKernelGGL(k_spk_lstm<S_H>, tiles, dim3(512), 0, ctx->stream, s->seq_b.p, S_H, P, (const spk_f4*)s->d_wp[2], s->d_bias[2], (float*)nullptr,
                       s->h_last.p);
    hipLaunchKernelGGL(k_spk_head, dim3(P), dim3(256), 0, ctx->stream, s->h_last.p, s->d_lin_w, s->d_lin_b, s->pemb.p);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

// The front end of n_clips clips up to the mel (and the clip / partial tables): validation first, then one launch per stage.
// h_flags[c] may be null (nothing is cut for that clip); with flags their count must be n16 / 480.
int spk_front(rt_spk* s, const char* who, const float* const* d_pcm, const int64_t* n_samples, int n_clips, int sr_in, const uint8_t* const* h_flags,
              const int32_t* n_flags, int* total_parts) {
    rt_ctx* ctx = s->ctx;
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "%s: the encoder is not finalized (rt_spk_finalize)", who);
    if (n_clips > 65535) return rt_fail(ctx, RT_ERR_INVALID, "%s: more than 65535 clips in one call", who);
    const bool resample = sr_in != S_SR;
    if (resample) RT_TRY(resampler_design(ctx, s->rs, sr_in, S_SR));
    s->h_clips.assign((size_t)n_clips, SpkClip{});
    s->h_win_dst.clear();
    s->h_part_row.clear();
    std::vector<int64_t> win_off((size_t)n_clips, -1);
    int64_t pcm_total = 0, pre_total = 0, frames_total = 0, parts_total = 0, max16 = 0, max_frames = 0;
    for (int c = 0; c < n_clips; ++c) {
        SpkClip& h = s->h_clips[c];
        if (!d_pcm[c] || n_samples[c] < 1) return rt_fail(ctx, RT_ERR_INVALID, "%s: clip %d is empty", who, c);
        h.pcm_in = d_pcm[c];
        h.n_in = n_samples[c];
        h.n16 = resample ? s->rs.n_out(h.n_in) : h.n_in;
        if (h.n16 < 1) return rt_fail(ctx, RT_ERR_INVALID, "%s: clip %d is empty at 16 kHz", who, c);
        h.n_pre = h.n16;
        if (h_flags && h_flags[c]) {
            const int64_t n_win = h.n16 / S_WIN;
            if (!n_flags || n_flags[c] != n_win)
                return rt_fail(ctx, RT_ERR_INVALID, "%s: clip %d has %lld windows of 480 samples at 16 kHz and %d voice flags", who, c, (long long)n_win,
                               n_flags ? n_flags[c] : -1);
            h.n_win = (int)n_win;
            win_off[c] = (int64_t)s->h_win_dst.size();
            s->h_win_dst.resize(s->h_win_dst.size() + (size_t)n_win + 1);       // (+ 1: a clip below 480 samples still has a table)
            h.n_pre = (int64_t)S_WIN * spk_smooth_flags(h_flags[c], (int)n_win, s->h_win_dst.data() + win_off[c]);
        }
        int parts = 0;
        spk_partials(h.n_pre, &parts, &h.n_pad);
        h.parts = parts;
        h.frames = (int)(1 + h.n_pad / S_HOP);
        h.first_frame = (int)frames_total;
        h.first_part = (int)parts_total;
        for (int i = 0; i < parts; ++i) s->h_part_row.push_back(h.first_frame + i * S_STEP);
        pcm_total += resample ? h.n16 : 0;
        pre_total += h.n_pad;
        frames_total += h.frames;
        parts_total += parts;
        max16 = std::max(max16, h.n16);
        max_frames = std::max<int64_t>(max_frames, h.frames);
        if (parts_total > S_MAX_PARTS) return rt_fail(ctx, RT_ERR_INVALID, "%s: more than %d partial utterances in one call", who, S_MAX_PARTS);
        if (frames_total > (int64_t)1 << 24) return rt_fail(ctx, RT_ERR_INVALID, "%s: more than 2^24 mel frames in one call", who);
    }
    if (resample) RT_TRY(spk_grow(ctx, s->pcm, (size_t)pcm_total));
    RT_TRY(spk_grow(ctx, s->pre, (size_t)pre_total));
    RT_TRY(spk_grow(ctx, s->mel, (size_t)frames_total * S_MELS));
    RT_TRY(spk_grow(ctx, s->parts, (size_t)parts_total * S_T * S_MELS));
    RT_TRY(spk_grow(ctx, s->scale, (size_t)n_clips));
    RT_TRY(spk_grow(ctx, s->win_dst, s->h_win_dst.size()));
    RT_TRY(spk_grow(ctx, s->part_row, (size_t)parts_total));
    RT_TRY(spk_grow(ctx, s->clips, (size_t)n_clips));
    int64_t off16 = 0, off_pre = 0;
    for (int c = 0; c < n_clips; ++c) {
        SpkClip& h = s->h_clips[c];
        h.pcm16 = resample ? s->pcm.p + off16 : h.pcm_in;
        h.pre = s->pre.p + off_pre;
        h.win_dst = win_off[c] >= 0 ? s->win_dst.p + win_off[c] : nullptr;
        off16 += resample ? h.n16 : 0;
        off_pre += h.n_pad;
    }
    RT_HIP(ctx, hipMemcpyAsync(s->clips.p, s->h_clips.data(), (size_t)n_clips * sizeof(SpkClip), hipMemcpyHostToDevice, ctx->stream));
    if (!s->h_win_dst.empty())
        RT_HIP(ctx, hipMemcpyAsync(s->win_dst.p, s->h_win_dst.data(), s->h_win_dst.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    RT_HIP(ctx, hipMemcpyAsync(s->part_row.p, s->h_part_row.data(), (size_t)parts_total * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    RT_HIP(ctx, hipMemsetAsync(s->pre.p, 0, (size_t)pre_total * sizeof(float), ctx->stream));
    const dim3 samples((unsigned)std::min<int64_t>((max16 + 255) / 256, 4096), n_clips);
    if (resample)
        hipLaunchKernelGGL(k_spk_resample, samples, dim3(256), 0, ctx->stream, s->clips.p, s->rs.L, s->rs.M, s->rs.taps, s->rs.half, s->rs.d_h);
    hipLaunchKernelGGL(k_spk_rms, dim3(n_clips), dim3(1024), 0, ctx->stream, s->clips.p, s->scale.p);
    hipLaunchKernelGGL(k_spk_scale_compact, samples, dim3(256), 0, ctx->stream, s->clips.p, s->scale.p);
    hipLaunchKernelGGL(k_spk_mel, dim3((unsigned)max_frames, n_clips), dim3(256), 0, ctx->stream, s->clips.p, s->d_win, s->d_twc, s->d_tws, s->d_melT,
                       s->mel.p);
    RT_HIP(ctx, hipGetLastError());
    *total_parts = (int)parts_total;
    return RT_OK;
}

void spk_free(rt_spk* s) {
    for (int l = 0; l < S_LAYERS; ++l)
        for (void* p : {(void*)s->d_wp[l], (void*)s->d_bias[l]})
            if (p) (void)hipFree(p);
    for (void* p : {(void*)s->d_lin_w, (void*)s->d_lin_b, (void*)s->d_melT, (void*)s->d_win, (void*)s->d_twc, (void*)s->d_tws, (void*)s->rs.d_h,
                    (void*)s->pcm.p, (void*)s->pre.p, (void*)s->mel.p, (void*)s->parts.p, (void*)s->seq_a.p, (void*)s->seq_b.p, (void*)s->h_last.p,
                    (void*)s->pemb.p, (void*)s->emb.p, (void*)s->scale.p, (void*)s->win_dst.p, (void*)s->part_row.p, (void*)s->clips.p})
        if (p) (void)hipFree(p);
}

}  // namespace

extern "C" {

int rt_spk_create(rt_ctx* ctx, rt_spk** out) {
    if (!ctx || !out) return rt_fail(ctx, RT_ERR_INVALID, "rt_spk_create: null argument");
    *out = nullptr;
    rt_spk* s = new rt_spk();
    s->ctx = ctx;
    *out = s;
    return RT_OK;
}

int rt_spk_destroy(rt_spk* s) {
    if (!s) return RT_OK;
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    spk_free(s);
    delete s;
    return RT_OK;
}

int rt_spk_set_tensor(rt_spk* s, const char* name, const float* h_data, int64_t rows, int64_t cols) {
    if (!s || !name || !h_data) return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_spk_set_tensor: null argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    if (s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_spk_set_tensor: the encoder is finalized");
    int64_t r = 0, c = 0;
    std::vector<float>* slot = spk_slot(s, name, &r, &c);
    if (!slot) return rt_fail(ctx, RT_ERR_INVALID, "rt_spk_set_tensor: no tensor named %s", name);
    if (rows != r || cols != c) return rt_fail(ctx, RT_ERR_INVALID, "rt_spk_set_tensor: %s is [%lld][%lld], got [%lld][%lld]", name, (long long)r, (long long)c,
                                               (long long)rows, (long long)cols);
    for (int64_t i = 0; i < r * c; ++i)
        if (!std::isfinite(h_data[i])) return rt_fail(ctx, RT_ERR_INVALID, "rt_spk_set_tensor: %s holds a value that is not finite", name);
    slot->assign(h_data, h_data + r * c);
    return RT_OK;
}

int rt_spk_finalize(rt_spk* s) {
    if (!s) return RT_ERR_INVALID;
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    if (s->finalized) return RT_OK;
    for (int l = 0; l < S_LAYERS; ++l)
        if (s->w_ih[l].empty() || s->w_hh[l].empty() || s->b_ih[l].empty() || s->b_hh[l].empty())
            return rt_fail(ctx, RT_ERR_STATE, "rt_spk_finalize: a tensor of LSTM layer %d is missing", l);
    if (s->lin_w.empty() || s->lin_b.empty() || s->melf.empty() || s->win.empty())
        return rt_fail(ctx, RT_ERR_STATE, "rt_spk_finalize: linear.weight, linear.bias, mel.filters or mel.window is missing");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    for (int l = 0; l < S_LAYERS; ++l) {
        const int kin = l == 0 ? S_MELS : S_H, kinp = l == 0 ? S_KIN0 : S_H, kt = kinp + S_H, nkg = kt / 16;
        std::vector<float> wp((size_t)S_G * kt), bias(S_G);
        // [hidden tile][gate][k group][lane][j] = [W_ih (zero-padded) | W_hh][gate 256 + 16 tile + (lane & 15)][16 kg + 4 (lane >> 4) + j]
        for (int ht = 0; ht < 16; ++ht)
            for (int g = 0; g < 4; ++g)
                for (int kg = 0; kg < nkg; ++kg)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 4; ++j) {
                            const int row = g * S_H + ht * 16 + (lane & 15), k = kg * 16 + (lane >> 4) * 4 + j;
                            float v = 0.0f;
                            if (k < kin) v = s->w_ih[l][(size_t)row * kin + k];
                            else if (k >= kinp) v = s->w_hh[l][(size_t)row * S_H + (k - kinp)];
                            wp[((((size_t)(ht * 4 + g) * nkg + kg) * 64) + lane) * 4 + j] = v;
                        }
        for (int i = 0; i < S_G; ++i) bias[i] = s->b_ih[l][i] + s->b_hh[l][i];
        RT_TRY(spk_upload(ctx, &s->d_wp[l], wp));
        RT_TRY(spk_upload(ctx, &s->d_bias[l], bias));
    }
    RT_TRY(spk_upload(ctx, &s->d_lin_w, s->lin_w));
    RT_TRY(spk_upload(ctx, &s->d_lin_b, s->lin_b));
    RT_TRY(spk_upload(ctx, &s->d_melT, s->melf));
    std::vector<double> win(S_NFFT), tc(S_NFFT), ts(S_NFFT);
    for (int i = 0; i < S_NFFT; ++i) {
        win[i] = (double)s->win[i];
        tc[i] = std::cos(2.0 * M_PI * i / S_NFFT);
        ts[i] = std::sin(2.0 * M_PI * i / S_NFFT);
    }
    RT_TRY(spk_upload(ctx, &s->d_win, win));
    RT_TRY(spk_upload(ctx, &s->d_twc, tc));
    RT_TRY(spk_upload(ctx, &s->d_tws, ts));
    for (int l = 0; l < S_LAYERS; ++l) { s->w_ih[l] = {}; s->w_hh[l] = {}; }
    s->finalized = true;
    return RT_OK;
}

int rt_spk_embed_batch(rt_spk* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips, int32_t sample_rate_in,
                       const uint8_t* const* h_voice_flags, const int32_t* n_voice_flags, float* h_embed, int32_t* h_n_partials) {
    if (!s || !d_pcm || !n_samples || n_clips < 1 || sample_rate_in < 1000 || !h_embed || !h_n_partials)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_spk_embed_batch: bad argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    int P = 0;
    RT_TRY(spk_front(s, "rt_spk_embed_batch", d_pcm, n_samples, n_clips, sample_rate_in, h_voice_flags, n_voice_flags, &P));
    hipLaunchKernelGGL(k_spk_gather, dim3(P), dim3(256), 0, ctx->stream, s->part_row.p, s->mel.p, s->parts.p);
    RT_TRY(spk_network(s, P));
    RT_TRY(spk_grow(ctx, s->emb, (size_t)n_clips * S_H));
    hipLaunchKernelGGL(k_spk_utter, dim3(n_clips), dim3(256), 0, ctx->stream, s->clips.p, s->pemb.p, s->emb.p);
    RT_HIP(ctx, hipGetLastError());
    RT_HIP(ctx, hipMemcpyAsync(h_embed, s->emb.p, (size_t)n_clips * S_H * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < n_clips; ++c) h_n_partials[c] = s->h_clips[c].parts;
    return RT_OK;
}

int rt_debug_spk_mel(rt_spk* s, const float* d_pcm, int64_t n_samples, int32_t sample_rate_in, const uint8_t* h_voice_flags, int32_t n_voice_flags,
                     float* h_mel, int32_t cap_frames, int32_t* h_n_frames, int64_t* h_n16) {
    if (!s || !d_pcm || sample_rate_in < 1000 || !h_mel || cap_frames < 1 || !h_n_frames || !h_n16)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_debug_spk_mel: bad argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    int P = 0;
    RT_TRY(spk_front(s, "rt_debug_spk_mel", &d_pcm, &n_samples, 1, sample_rate_in, h_voice_flags ? &h_voice_flags : nullptr, &n_voice_flags, &P));
    const SpkClip& c = s->h_clips[0];
    if (c.frames > cap_frames) {
        (void)hipStreamSynchronize(ctx->stream);
        return rt_fail(ctx, RT_ERR_LENGTH, "rt_debug_spk_mel: %d mel frames, room for %d", c.frames, cap_frames);
    }
    RT_HIP(ctx, hipMemcpyAsync(h_mel, s->mel.p, (size_t)c.frames * S_MELS * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *h_n_frames = c.frames;
    *h_n16 = c.n_pre;
    return RT_OK;
}

int rt_debug_spk_lstm(rt_spk* s, const float* h_partials, int32_t n_partials, float* h_embed) {
    if (!s || !h_partials || !h_embed || n_partials < 1 || n_partials > S_MAX_PARTS)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_debug_spk_lstm: bad argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    if (!s->finalized) return rt_fail(ctx, RT_ERR_STATE, "rt_debug_spk_lstm: the encoder is not finalized (rt_spk_finalize)");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)n_partials * S_T * S_MELS;
    RT_TRY(spk_grow(ctx, s->parts, n));
    RT_HIP(ctx, hipMemcpyAsync(s->parts.p, h_partials, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    RT_TRY(spk_network(s, n_partials));
    RT_HIP(ctx, hipMemcpyAsync(h_embed, s->pemb.p, (size_t)n_partials * S_H * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

}  // extern "C"
