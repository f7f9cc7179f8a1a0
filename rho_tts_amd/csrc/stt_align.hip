// Token times by dynamic time warping over cross-attention (rt_stt_align; DESIGN.md section 5, "word times"): the kernels behind the
// teacher-forced decoder pass of csrc/stt.hip.  Whisper's method (openai/whisper timing.py; transformers' generation_whisper.py
// _extract_token_timestamps): the cross-attention probabilities of a few alignment heads are normalised over the tokens, median-filtered
// along time, averaged over the heads, and the monotone token-to-frame path of least cost -M is found by dynamic time warping.
//
//   k_stt_align_probs    per (alignment row, alignment head): softmax over all encoder positions of q . k / sqrt(d), as the layer's own
//                        attention forms it (q from the layer's q buffer, K from the cross-attention cache's planes), t < F written
//   k_stt_align_logprob  per alignment row: log_softmax over the text ids of the row's logits at the token the row predicts
//   k_stt_align_stats    per (window, head, frame): mean and population standard deviation over the rows, float64 in row order
//   k_stt_align_matrix   per (window, row, frame): z = (w - mean) / std (0 where std is 0), median along time under reflect padding,
//                        mean over the heads in float64, rounded once
//   k_stt_dtw            one workgroup per window: anti-diagonal sweep of the cost table in float32, 2-bit trace, backtrace on one lane
//
// Every reduction has a fixed order, and no launch mixes windows: a window's results do not depend on what it is batched with.
#include <algorithm>

#include "kernels.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned au4_t;

template <int D>
__global__ __launch_bounds__(256) void k_stt_align_probs(const float* __restrict__ q, int heads, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ kc_lo,
                                                         int n_ctx, AlignRows rows, AlignHeads hs, int64_t head_stride, float* __restrict__ W) {
    extern __shared__ float sc[];                          // [n_ctx] the row's scores
    __shared__ float red[4];
    const int a = blockIdx.x, hh = blockIdx.y, h = hs.head[hh], tid = threadIdx.x, wave = tid >> 6;
    const int row = rows.src[a], slot = rows.slot[a], F = min(rows.frames[a], n_ctx);
    const float scale = rsqrtf((float)D);
    float qr[D];
#pragma unroll
    for (int j = 0; j < D; ++j) qr[j] = q[((int64_t)row * heads + h) * D + j] * scale;
    const int64_t base = ((int64_t)slot * heads + h) * n_ctx * D;
    float m = -INFINITY;
    for (int t = tid; t < n_ctx; t += 256) {
        const au4_t* k4 = reinterpret_cast<const au4_t*>(kc + base + (int64_t)t * D);
        const au4_t* l4 = kc_lo ? reinterpret_cast<const au4_t*>(kc_lo + base + (int64_t)t * D) : nullptr;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < D / 8; ++c) {
            const au4_t kv = k4[c];
            au4_t lv = {0u, 0u, 0u, 0u};
            if (l4) lv = l4[c];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float k0 = __uint_as_float(kv[j] << 16) + __uint_as_float(lv[j] << 16);
                const float k1 = __uint_as_float(kv[j] & 0xffff0000u) + __uint_as_float(lv[j] & 0xffff0000u);
                s += qr[c * 8 + 2 * j] * k0;
                s += qr[c * 8 + 2 * j + 1] * k1;
            }
        }
        sc[t] = s;
        m = fmaxf(m, s);
    }
    m = wave_max_f32(m);
    if ((tid & 63) == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    // the sum in a fixed order: per thread in index order, butterfly per wave, the four wave sums in wave order
    float sum = 0.f;
    for (int t = tid; t < n_ctx; t += 256) sum += expf(sc[t] - m);
    sum = wave_sum_f32(sum);
    if ((tid & 63) == 0) red[wave] = sum;
    __syncthreads();
    sum = ((red[0] + red[1]) + red[2]) + red[3];
    float* o = W + rows.out[a] + (int64_t)hs.out[hh] * head_stride;
    for (int t = tid; t < F; t += 256) o[t] = expf(sc[t] - m) / sum;
}

__global__ __launch_bounds__(1024) void k_stt_align_logprob(const float* __restrict__ logits, int V, const int32_t* __restrict__ tok, int hi, float* __restrict__ out) {
    __shared__ float red[16];
    const float* x = logits + (int64_t)blockIdx.x * V;
    const int tid = threadIdx.x, wave = tid >> 6;
    float m = -INFINITY;
    for (int i = tid; i < hi; i += 1024) m = fmaxf(m, x[i]);
    m = wave_max_f32(m);
    if ((tid & 63) == 0) red[wave] = m;
    __syncthreads();
    m = red[0];
    for (int k = 1; k < 16; ++k) m = fmaxf(m, red[k]);
    __syncthreads();
    float sum = 0.f;
    for (int i = tid; i < hi; i += 1024) sum += expf(x[i] - m);
    sum = wave_sum_f32(sum);
    if ((tid & 63) == 0) red[wave] = sum;
    __syncthreads();
    if (tid != 0) return;
    sum = red[0];
    for (int k = 1; k < 16; ++k) sum += red[k];
    const int t = min(max(tok[blockIdx.x], 0), hi - 1);
    out[blockIdx.x] = x[t] - (m + logf(sum));
}

// blockIdx = (frame block, head, window)
__global__ __launch_bounds__(256) void k_stt_align_stats(const float* __restrict__ W, const AlignWin* __restrict__ wins, int n_heads, int64_t head_stride, int ldw,
                                                         double* __restrict__ stats) {
    const AlignWin win = wins[blockIdx.z];
    const int h = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= win.F) return;
    const float* p = W + win.w_off + (int64_t)h * head_stride + t;
    double s = 0.0;
    for (int r = 0; r < win.n; ++r) s += (double)p[(int64_t)r * ldw];
    const double mean = s / (double)win.n;
    double v = 0.0;
    for (int r = 0; r < win.n; ++r) { const double d = (double)p[(int64_t)r * ldw] - mean; v += d * d; }
    double* o = stats + 2 * (((int64_t)blockIdx.z * n_heads + h) * ldw + t);
    o[0] = mean;
    o[1] = sqrt(v / (double)win.n);
}

// blockIdx = (frame block, row, window)
__global__ __launch_bounds__(256) void k_stt_align_matrix(const float* __restrict__ W, const AlignWin* __restrict__ wins, int n_heads, int64_t head_stride, int ldw,
                                                          int width, const double* __restrict__ stats, float* __restrict__ M) {
    const AlignWin win = wins[blockIdx.z];
    const int r = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    if (r >= win.n || t >= win.F) return;
    const int pad = width / 2;
    const bool filter = win.F > pad;                       // (a window of at most width / 2 frames is not filtered: the reference's rule)
    double acc = 0.0;
    for (int h = 0; h < n_heads; ++h) {
        const float* p = W + win.w_off + (int64_t)h * head_stride + (int64_t)r * ldw;
        const double* st = stats + 2 * (((int64_t)blockIdx.z * n_heads + h) * ldw);
        auto z = [&](int i) -> double {
            const double sd = st[2 * i + 1];
            return sd == 0.0 ? 0.0 : ((double)p[i] - st[2 * i]) / sd;       // (a constant column: 0 where the reference has NaN)
        };
        if (!filter) { acc += z(t); continue; }
        double buf[ALIGN_MEDIAN_MAX];
        for (int k = 0; k < width; ++k) {
            int i = t - pad + k;
            if (i < 0) i = -i;                             // reflect, no edge repeat
            if (i >= win.F) i = 2 * (win.F - 1) - i;
            const double v = z(i);
            int at = k;
            for (; at > 0 && buf[at - 1] > v; --at) buf[at] = buf[at - 1];
            buf[at] = v;
        }
        acc += buf[pad];
    }
    M[win.m_off + (int64_t)r * win.F + t] = (float)(acc / (double)n_heads);
}

// One workgroup per window.  Cell (i, j), 1 <= i <= n, 1 <= j <= F, of the cost table lies on anti-diagonal i + j and needs the two
// diagonals before it, kept in LDS (three lines of `ld` floats, rotating; the borders are not stored: cost[0][0] = 0, the rest of row 0
// and of column 0 is +inf).  Row i belongs to one thread throughout, and its trace cells lie in words of its own: no two threads ever
// write one word.  The choice rule is the reference's, ties included: diagonal if c0 < c1 && c0 < c2, else up if c1 < c0 && c1 < c2,
// else left.  cost = -M + min in float32 (equal to the reference's float64 sum rounded to float32: 53 >= 2 * 24 + 2).
__global__ __launch_bounds__(512) void k_stt_dtw(const float* __restrict__ M, const AlignWin* __restrict__ wins, int ld, uint32_t* __restrict__ g_trace, int in_lds,
                                                 int32_t* __restrict__ frames) {
    extern __shared__ uint32_t sh[];
    const AlignWin win = wins[blockIdx.x];
    const int N = win.n, F = win.F, tid = threadIdx.x;
    if (N < 1 || F < 1 || N + 1 > ld) return;              // (uniform)
    float* dg = reinterpret_cast<float*>(sh);
    const int Wd = (F + 16) / 16;                          // words of a row: cells j = 0 .. F
    uint32_t* tr = in_lds ? sh + 3 * ld : g_trace + win.t_off;
    for (int i = tid; i < (N + 1) * Wd; i += 512) tr[i] = 0u;
    __syncthreads();
    const float* Mw = M + win.m_off;
    for (int d = 2; d <= N + F; ++d) {
        float* cur = dg + (d % 3) * ld;
        const float* p1 = dg + ((d - 1) % 3) * ld;
        const float* p2 = dg + ((d - 2) % 3) * ld;
        const int ilo = max(1, d - F), ihi = min(N, d - 1);
        for (int i = 1 + tid; i <= ihi; i += 512) {
            if (i < ilo) continue;
            const int j = d - i;
            const float c0 = (i == 1 || j == 1) ? ((i == 1 && j == 1) ? 0.f : INFINITY) : p2[i - 1];
            const float c1 = i == 1 ? INFINITY : p1[i - 1];
            const float c2 = j == 1 ? INFINITY : p1[i];
            float c;
            uint32_t t;
            if (c0 < c1 && c0 < c2) { c = c0; t = 0u; }
            else if (c1 < c0 && c1 < c2) { c = c1; t = 1u; }
            else { c = c2; t = 2u; }
            cur[i] = -Mw[(int64_t)(i - 1) * F + (j - 1)] + c;
            tr[i * Wd + (j >> 4)] |= t << ((j & 15) * 2);
        }
        __syncthreads();
    }
    if (tid != 0) return;
    // the path back from (N, F); row 0 reads "left" and column 0 reads "up".  A row's entry is overwritten until the path leaves it:
    // what stays is the frame at which the forward path first enters the row (the reference's time_indices[jumps])
    int32_t* out = frames + win.f_off;
    int i = N, j = F;
    for (int guard = 0; guard <= N + F + 1 && (i > 0 || j > 0); ++guard) {
        if (i >= 1) out[i - 1] = j - 1;
        const uint32_t t = i == 0 ? 2u : (j == 0 ? 1u : (tr[i * Wd + (j >> 4)] >> ((j & 15) * 2)) & 3u);
        if (t == 0u) { --i; --j; }
        else if (t == 1u) --i;
        else --j;
    }
}

constexpr size_t ALIGN_DTW_LDS_MAX = 152 * 1024;           // of the 160 KB a workgroup may hold

}  // namespace

int launch_align_probs(rt_ctx* ctx, const float* q, int heads, int head_dim, const KvCache& cross, int layer, const AlignRows& rows, int n_rows, const AlignHeads& hs,
                       int64_t head_stride, float* W) {
    if (n_rows <= 0 || hs.n <= 0) return RT_OK;
    if (hs.n > ALIGN_HEADS_MAX || cross.kv_heads != heads || cross.head_dim != head_dim || layer < 0 || layer >= cross.layers)
        return rt_fail(ctx, RT_ERR_INVALID, "align: the heads do not fit the cross-attention cache");
    const bf16_t* kc = cross.k + (size_t)layer * cross.layer_stride();
    const bf16_t* kl = cross.k_lo ? cross.k_lo + (size_t)layer * cross.layer_stride() : nullptr;
    const dim3 grid(n_rows, hs.n);
    const size_t lds = (size_t)cross.max_pos * sizeof(float);
    if (lds > 60 * 1024) return rt_fail(ctx, RT_ERR_UNSUPPORTED, "align: %d encoder positions do not fit the score line", cross.max_pos);
    switch (head_dim) {
        case 32: hipLaunchKernelGGL(k_stt_align_probs<32>, grid, dim3(256), lds, ctx->stream, q, heads, kc, kl, cross.max_pos, rows, hs, head_stride, W); break;
        case 64: hipLaunchKernelGGL(k_stt_align_probs<64>, grid, dim3(256), lds, ctx->stream, q, heads, kc, kl, cross.max_pos, rows, hs, head_stride, W); break;
        case 128: hipLaunchKernelGGL(k_stt_align_probs<128>, grid, dim3(256), lds, ctx->stream, q, heads, kc, kl, cross.max_pos, rows, hs, head_stride, W); break;
        default: return rt_fail(ctx, RT_ERR_UNSUPPORTED, "align: head_dim %d unsupported (32, 64, 128)", head_dim);
    }
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

int launch_align_logprob(rt_ctx* ctx, const float* logits, int V, int n_rows, const int32_t* tok, int hi, float* out) {
    if (n_rows <= 0) return RT_OK;
    if (hi < 1 || hi > V) return rt_fail(ctx, RT_ERR_INVALID, "align: text ids [0, %d) outside the vocabulary of %d", hi, V);
    hipLaunchKernelGGL(k_stt_align_logprob, dim3(n_rows), dim3(1024), 0, ctx->stream, logits, V, tok, hi, out);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

int launch_align_matrix(rt_ctx* ctx, const float* W, const AlignWin* d_wins, int n_win, int n_heads, int64_t head_stride, int ldw, int max_n, int max_F, int width,
                        double* stats, float* M) {
    if (n_win <= 0 || max_n <= 0 || max_F <= 0) return RT_OK;
    if (n_heads < 1 || n_heads > ALIGN_HEADS_MAX || width < 1 || width > ALIGN_MEDIAN_MAX || !(width & 1) || max_F > ldw || max_n > 65535 || n_win > 65535)
        return rt_fail(ctx, RT_ERR_INVALID, "align: 1 .. %d heads and an odd median width of 1 .. %d", ALIGN_HEADS_MAX, ALIGN_MEDIAN_MAX);
    const unsigned fb = (unsigned)((max_F + 255) / 256);
    hipLaunchKernelGGL(k_stt_align_stats, dim3(fb, n_heads, n_win), dim3(256), 0, ctx->stream, W, d_wins, n_heads, head_stride, ldw, stats);
    hipLaunchKernelGGL(k_stt_align_matrix, dim3(fb, max_n, n_win), dim3(256), 0, ctx->stream, W, d_wins, n_heads, head_stride, ldw, width, stats, M);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

int launch_align_dtw(rt_ctx* ctx, const float* M, const AlignWin* d_wins, int n_win, int max_n, int max_F, uint32_t* d_trace, int trace_mode, int32_t* frames) {
    if (n_win <= 0 || max_n <= 0 || max_F <= 0) return RT_OK;
    const int ld = max_n + 1;
    const size_t diag = (size_t)3 * ld * sizeof(float), full = diag + align_trace_words(max_n, max_F) * sizeof(uint32_t);
    bool in_lds = trace_mode != 0 && full <= ALIGN_DTW_LDS_MAX;
    if (trace_mode == 1 && !in_lds) return rt_fail(ctx, RT_ERR_INVALID, "align: a trace of %zu bytes does not fit the LDS", full);
    if (diag > ALIGN_DTW_LDS_MAX) return rt_fail(ctx, RT_ERR_LENGTH, "align: %d rows do not fit the path kernel", max_n);
    if (in_lds && full > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(k_stt_dtw), hipFuncAttributeMaxDynamicSharedMemorySize, (int)full) != hipSuccess) {
        (void)hipGetLastError();
        if (trace_mode == 1) return rt_fail(ctx, RT_ERR_UNSUPPORTED, "align: the device refuses %zu bytes of LDS", full);
        in_lds = false;
    }
    if (!in_lds && !d_trace) return rt_fail(ctx, RT_ERR_INVALID, "align: the trace needs a global scratch");
    hipLaunchKernelGGL(k_stt_dtw, dim3(n_win), dim3(512), in_lds ? full : diag, ctx->stream, M, d_wins, ld, d_trace, in_lds ? 1 : 0, frames);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}
