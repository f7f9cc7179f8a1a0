// Hand-crafted drift-classifier features from a waveform that already lives in HBM.
// Stands behind the front half of validation/classifier/trainer.py:23-96 (extract_features / _estimate_formants): what the
// reference computes with librosa on a temporary WAV - 13 MFCCs per frame, the pYIN difference function, a Burg LPC of the
// mid-file frame - is computed where the generated segment is, and only a few kilobytes leave the GPU:
//
//   PCM at the TTS rate -> windowed-sinc resampler (16 kHz; resample.h, the resampler of the speech-to-text front-end)
//     -> MFCC: frames of 2048 (hop 512, zero-padded centre), periodic Hann, 2048-point DFT in float64, power spectrum,
//        128 slaney mel filters, 10 log10 (floor 1e-10), max - 80 dB floor, DCT-II (orthonormal) rows 0..12 -> mean and
//        standard deviation of every coefficient over the frames (26 numbers)
//     -> pYIN front half: per frame d(tau) = sum_{j=1..1024} (x[j] - x[j + tau])^2, cumulative-mean-normalised, for the lags
//        min_period .. max_period ([frames][lags] float64)
//     -> pYIN back half (rt_features_extract_batch only; the single-clip call hands the difference function to the host functions
//        of rho_tts_amd/features.py, which are the reference definition of both kernels): trough statistics -> log observation
//        probabilities [frames][2 n_bins] (k_feat_observe), Viterbi pass over the 2 n_bins states, one workgroup per clip
//        (k_feat_viterbi) -> one state per pitch frame
//     -> LPC: pre-emphasis 0.97 in float32, 400-sample symmetric-Hann frame about the middle sample, Burg's recursion in
//        float64 -> order + 1 coefficients (their roots - an 18 x 18 eigenproblem - are taken on the host)
//
// There is one path (feat_run).  rt_features_extract is it with one clip and no back half, rt_features_extract_batch with a whole
// validation chunk: a small device table (FeatClip, one entry per clip) tells every kernel where a clip's samples and frames are, and
// each stage is ONE launch for the call - blockIdx.y (blockIdx.x for the per-clip kernels k_feat_stats and k_feat_lpc) is the clip,
// the grid is sized by the longest clip and the rows past a clip's own count return at once.  No launch mixes clips and every
// workgroup does for its clip what it does when the clip is alone, so a clip's bits do not depend on its neighbours or on the entry
// point (tests/test_features_bits_gpu.py holds both to recorded bits).  The handle holds one workspace set, grown on demand.
//
// Nothing here is on the hot path of generation (one call per validated segment, ~0.3 ms of GPU time for 3.5 s of audio), so
// the kernels are the simple forms: direct DFT and direct difference sums in float64, one workgroup per frame.
// PARITY UNPINNED (librosa absent): the definitions are those of oracle/features.py, which restates librosa 0.10's defaults.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "kernels.h"
#include "resample.h"

// One clip of a call, as the kernels see it (a small device table, one entry per clip; rt_debug_features_viterbi fills it with null audio)
struct FeatClip {
    const float* pcm_in;    // the clip's samples at the input rate
    const float* pcm16;     // ... at 16 kHz: its stretch of the resampler's output, or pcm_in itself when the rates agree
    int64_t n_in, n16;
    int32_t first, frames;  // first frame of the clip in the frame-major workspaces of the call, and its frame count
};

template <class T>
struct FeatBuf { T* p = nullptr; size_t cap = 0; };

struct rt_features {
    rt_ctx* ctx = nullptr;
    // tables
    double *d_twc = nullptr, *d_tws = nullptr;     // cos / sin(2 pi n / 2048)
    float* d_melT = nullptr;                       // [1025][128]
    double* d_dct = nullptr;                       // [13][128]
    Resampler rs;                                  // (sample_rate_in -> 16 kHz) of the last call that needed one
    // pYIN's back half (rt_features_set_pitch_model): every table comes from the host, so the device compares and adds the host's bits
    bool pm_set = false;
    int pm_bins = 0, pm_hw = 0, pm_thr = 0;
    double *pm_d_thr = nullptr, *pm_d_beta = nullptr;          // [n_thresholds] each
    double *pm_d_trans = nullptr, *pm_d_init = nullptr;        // [2][2 hw + 1][n_bins] (stay, switch), [2 n_bins]
    double pm_log_tiny = 0.0, pm_sr = 0.0, pm_fmin = 0.0, pm_bins_per_octave = 0.0, pm_no_trough = 0.0;
    // the one workspace set (every entry point), sized by the call, grown on demand (feat_grow); "frames" = those of all clips of the call
    FeatBuf<float> pcm, logmel;                    // every clip at 16 kHz, back to back; [frames][128]
    FeatBuf<double> mfcc, cmnd, logobs;            // [frames][13], [frames][lags], [frames][2 n_bins]
    FeatBuf<int> ptr, states, gmax;                // Viterbi backpointers [frames][2 n_bins], state paths [clips][stride], [clips]
    FeatBuf<double> stats, lpc;                    // [clips][26], [clips][order + 1]
    FeatBuf<FeatClip> clips;                       // the clip table of the call, and its host copy
    std::vector<FeatClip> h_clips;
};

namespace {

constexpr int F_SR = 16000, F_NFFT = 2048, F_HOP = 512, F_BINS = F_NFFT / 2 + 1, F_MELS = 128, F_MFCC = 13;
constexpr int P_FRAME = 2048, P_WIN = 1024, P_HOP = 512;
constexpr int LPC_MAX = 32, LPC_FRAME = 400;

// Every front-half kernel begins with its clip's entry of the table: blockIdx.y (blockIdx.x in the two per-clip kernels) is the clip,
// and a frame past the clip's own count returns at once, uniformly over the workgroup.  Behind that each body is what it is for a
// clip alone: the same loads and sums in the same order.

// The resampler (resample.h) over the clips of a call; with a resampler every pcm16 lies in the handle's own buffer, and this is its writer
__global__ void k_feat_resample(const FeatClip* __restrict__ clips, int L, int M, int taps, int half, const float* __restrict__ h) {
    const FeatClip c = clips[blockIdx.y];
    float* y = const_cast<float*>(c.pcm16);
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < c.n16; n += (int64_t)gridDim.x * blockDim.x)
        y[n] = resample_at(c.pcm_in, c.n_in, n, L, M, taps, half, h);
}

// One MFCC frame per workgroup: frame f covers samples [f hop - 1024, f hop + 1024) of the signal (zeros outside), times the periodic
// Hann window; bin k on thread k (+ 256 i): direct DFT with the twiddle index k n mod 2048; mel filters; 10 log10.  gmax is [clips].
__global__ __launch_bounds__(256) void k_feat_logmel(const FeatClip* __restrict__ clips, const double* __restrict__ twc, const double* __restrict__ tws,
                                                     const float* __restrict__ melT, float* __restrict__ logmel, int* __restrict__ gmax) {
    extern __shared__ double fsh[];               // xw[2048] | c[2048] | s[2048] | power[1025]
    const FeatClip clip = clips[blockIdx.y];
    if ((int)blockIdx.x >= clip.frames) return;
    const float* __restrict__ pcm = clip.pcm16;
    const int64_t n = clip.n16;
    logmel += (int64_t)clip.first * F_MELS;
    gmax += blockIdx.y;
    double* xw = fsh;
    double* tc = fsh + F_NFFT;
    double* ts = tc + F_NFFT;
    double* pw = ts + F_NFFT;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int64_t start = (int64_t)f * F_HOP - F_NFFT / 2;
    for (int i = tid; i < F_NFFT; i += 256) {
        const int64_t t = start + i;
        const double v = (t >= 0 && t < n) ? (double)pcm[t] : 0.0;
        tc[i] = twc[i];
        ts[i] = tws[i];
        xw[i] = v * (0.5 - 0.5 * tc[i]);          // periodic Hann: 0.5 - 0.5 cos(2 pi i / 2048)
    }
    __syncthreads();
    for (int k = tid; k < F_BINS; k += 256) {
        double re = 0.0, im = 0.0;
        int idx = 0;
        for (int i = 0; i < F_NFFT; ++i) {
            re += xw[i] * tc[idx];
            im -= xw[i] * ts[idx];
            idx = (idx + k) & (F_NFFT - 1);
        }
        pw[k] = re * re + im * im;
    }
    __syncthreads();
    float best = -INFINITY;
    for (int m = tid; m < F_MELS; m += 256) {
        double acc = 0.0;
        for (int k = 0; k < F_BINS; ++k) acc += (double)melT[(int64_t)k * F_MELS + m] * pw[k];
        const float v = (float)(10.0 * log10(fmax(acc, 1e-10)));
        logmel[(int64_t)f * F_MELS + m] = v;
        best = fmaxf(best, v);
    }
    best = wave_max_f32(best);
    if ((tid & 63) == 0 && best > -INFINITY) atomicMax(gmax, f32_ordered(best));
}

// mfcc[f][c] = sum_m dct[c][m] max(logmel[f][m], gmax - 80): one frame per workgroup of 64 threads (13 of them busy: tiny)
__global__ __launch_bounds__(64) void k_feat_dct(const FeatClip* __restrict__ clips, const float* __restrict__ logmel, const int* __restrict__ gmax,
                                                 const double* __restrict__ dct, double* __restrict__ mfcc) {
    const FeatClip clip = clips[blockIdx.y];
    if ((int)blockIdx.x >= clip.frames) return;
    logmel += (int64_t)clip.first * F_MELS;
    mfcc += (int64_t)clip.first * F_MFCC;
    gmax += blockIdx.y;
    const int f = blockIdx.x, c = threadIdx.x;
    if (c >= F_MFCC) return;
    const float floor_db = ordered_f32(*gmax) - 80.0f;
    double acc = 0.0;
    for (int m = 0; m < F_MELS; ++m) acc += dct[c * F_MELS + m] * (double)fmaxf(logmel[(int64_t)f * F_MELS + m], floor_db);
    mfcc[(int64_t)f * F_MFCC + c] = acc;
}

// stats[c] = mean over the frames, stats[13 + c] = population standard deviation (np.std, ddof 0); one wave per (clip, coefficient)
__global__ __launch_bounds__(64) void k_feat_stats(const FeatClip* __restrict__ clips, const double* __restrict__ mfcc, double* __restrict__ stats) {
    const int n_frames = clips[blockIdx.x].frames;
    mfcc += (int64_t)clips[blockIdx.x].first * F_MFCC;
    stats += (int64_t)blockIdx.x * 2 * F_MFCC;
    const int c = blockIdx.y, lane = threadIdx.x;
    double s = 0.0;
    for (int f = lane; f < n_frames; f += 64) s += mfcc[(int64_t)f * F_MFCC + c];
    const double mean = wave_sum_f64(s) / (double)n_frames;
    double q = 0.0;
    for (int f = lane; f < n_frames; f += 64) { const double d = mfcc[(int64_t)f * F_MFCC + c] - mean; q += d * d; }
    q = wave_sum_f64(q);
    if (lane == 0) { stats[c] = mean; stats[F_MFCC + c] = sqrt(q / (double)n_frames); }
}

// One pitch frame per workgroup: x = samples [f hop - 1024, f hop + 1024) (zeros outside); d(tau) = sum_{j=1..1024} (x[j] - x[j+tau])^2
// for tau = 1 .. max_p (thread tau), prefix mean of d over 1 .. tau, out[f][tau - min_p] = d(tau) / (mean + tiny).
__global__ __launch_bounds__(512) void k_feat_cmnd(const FeatClip* __restrict__ clips, int min_p, int max_p, double* __restrict__ out) {
    __shared__ double x[P_FRAME];
    __shared__ double d[1024 + 1];
    const FeatClip clip = clips[blockIdx.y];
    if ((int)blockIdx.x >= clip.frames) return;
    const float* __restrict__ pcm = clip.pcm16;
    const int64_t n = clip.n16;
    out += (int64_t)clip.first * (max_p - min_p + 1);
    const int f = blockIdx.x, tid = threadIdx.x;
    const int64_t start = (int64_t)f * P_HOP - P_FRAME / 2;
    for (int i = tid; i < P_FRAME; i += 512) {
        const int64_t t = start + i;
        x[i] = (t >= 0 && t < n) ? (double)pcm[t] : 0.0;
    }
    __syncthreads();
    for (int tau = 1 + tid; tau <= max_p; tau += 512) {
        double acc = 0.0;
        for (int j = 1; j <= P_WIN; ++j) { const double e = x[j] - x[j + tau]; acc += e * e; }
        d[tau] = acc;
    }
    __syncthreads();
    if (tid == 0) {                                 // running sums in lag order (338 additions: the order the oracle's cumsum takes)
        double run = 0.0;
        for (int tau = 1; tau <= max_p; ++tau) {
            run += d[tau];
            if (tau >= min_p) out[(int64_t)f * (max_p - min_p + 1) + (tau - min_p)] = d[tau] / (run / (double)tau + 2.2250738585072014e-308);
        }
    }
}

// Burg's recursion (Marple) on the pre-emphasised, symmetric-Hann-windowed 25-ms frame about the middle sample; one wave.
__global__ __launch_bounds__(64) void k_feat_lpc(const FeatClip* __restrict__ clips, int order, double* __restrict__ a_out) {
    __shared__ double fwd[LPC_FRAME], bwd[LPC_FRAME], a[LPC_MAX + 1], prev[LPC_MAX + 1];
    const float* __restrict__ pcm = clips[blockIdx.x].pcm16;
    const int64_t n = clips[blockIdx.x].n16;
    a_out += (int64_t)blockIdx.x * (order + 1);
    const int lane = threadIdx.x;
    const int64_t c = n / 2;
    const int64_t lo = c - LPC_FRAME / 2 > 0 ? c - LPC_FRAME / 2 : 0, hi = c + LPC_FRAME / 2 < n ? c + LPC_FRAME / 2 : n;
    const int len = (int)(hi - lo);
    if (len < 2) { if (lane <= order) a_out[lane] = lane == 0 ? 1.0 : 0.0; return; }
    // frame[i] = y_pre[lo + i] * hanning(len)[i], y_pre[0] = y[0], y_pre[t] = y[t] - 0.97f y[t-1] in float32
    for (int i = lane; i < len; i += 64) {
        const int64_t t = lo + i;
        const float yp = t == 0 ? pcm[0] : pcm[t] - 0.97f * pcm[t - 1];
        const double w = len > 1 ? 0.5 - 0.5 * cos(2.0 * M_PI * (double)i / (double)(len - 1)) : 1.0;
        const double v = (double)yp * w;
        if (i >= 1) fwd[i - 1] = v;
        if (i < len - 1) bwd[i] = v;
    }
    for (int i = lane; i <= LPC_MAX; i += 64) { a[i] = i == 0 ? 1.0 : 0.0; prev[i] = a[i]; }
    __syncthreads();
    int m = len - 1;                                // live length of fwd / bwd
    double den;
    {
        double s = 0.0;
        for (int i = lane; i < m; i += 64) s += fwd[i] * fwd[i] + bwd[i] * bwd[i];
        den = wave_sum_f64(s);
    }
    double* pa = a;
    double* pp = prev;
    for (int it = 0; it < order && m > 0; ++it) {
        double s = 0.0;
        for (int i = lane; i < m; i += 64) s += bwd[i] * fwd[i];
        const double k = -2.0 * wave_sum_f64(s) / (den + 2.2250738585072014e-308);
        double* t = pa; pa = pp; pp = t;            // a <-> prev
        for (int j = 1 + lane; j <= it + 1; j += 64) pa[j] = pp[j] + k * pp[it - j + 1];
        if (lane == 0) pa[0] = 1.0;
        // fwd <- fwd + k bwd, bwd <- bwd + k fwd(old); then drop fwd[0] and bwd[last]
        double f0v = 0.0, blast = 0.0;
        for (int i = lane; i < m; i += 64) {
            const double fo = fwd[i], bo = bwd[i];
            const double fn = fo + k * bo, bn = bo + k * fo;
            if (i == 0) f0v = fn;
            if (i == m - 1) blast = bn;
            bwd[i] = bn;
            fwd[i] = fn;
        }
        f0v = wave_sum_f64(f0v);
        blast = wave_sum_f64(blast);
        den = (1.0 - k * k) * den - blast * blast - f0v * f0v;
        __syncthreads();
        // shift fwd down by one (fwd = fwd[1:]); bwd = bwd[:-1] is a shorter live length only
        double keep[(LPC_FRAME + 63) / 64];
        int q = 0;
        for (int i = lane; i + 1 < m; i += 64) keep[q++] = fwd[i + 1];
        __syncthreads();
        q = 0;
        for (int i = lane; i + 1 < m; i += 64) fwd[i] = keep[q++];
        __syncthreads();
        --m;
    }
    __syncthreads();
    for (int i = lane; i <= order; i += 64) a_out[i] = pa[i];
}

// ---- pYIN's back half.  The definitions are the host functions of rho_tts_amd/features.py, point by point: observation_log_probs
// for k_feat_observe, viterbi_banded for k_feat_viterbi.
constexpr double F_TINY = 2.2250738585072014e-308;

// One pitch frame per workgroup: cmnd[f][0 .. n_lags) -> out[f][0 .. 2 n_bins) = log(observation + tiny).
// Troughs are compacted in ascending lag by one wave (ballot).  The thresholds ascend, so "trough i is below threshold k" holds
// exactly for k >= k0[i], the first threshold above its height (found with the host's own comparison h < thr[k] on the uploaded
// thresholds): the count of troughs below threshold k is #{i : k0[i] <= k}, the rank of trough i among them #{i' < i : k0[i'] <= k}.
// Dynamic LDS: c[n_lags] | obs[n_bins] | h[mcap] | pr[mcap] (doubles) | idx[mcap] | k0[mcap] | bin[mcap] | nk[n_thr] (ints),
// mcap = (n_lags + 1) / 2 + 1 (two neighbouring lags cannot both be troughs).
__global__ __launch_bounds__(256) void k_feat_observe(const double* __restrict__ cmnd, int n_lags, int min_p, int n_bins, int n_thr,
                                                      const double* __restrict__ thr, const double* __restrict__ beta, double pitch_sr, double f_min,
                                                      double bins_per_octave, double no_trough, double* __restrict__ out) {
    extern __shared__ double osh[];
    const int mcap = (n_lags + 1) / 2 + 1;
    double* c = osh;
    double* obs = c + n_lags;
    double* h = obs + n_bins;
    double* pr = h + mcap;
    int* idx = (int*)(pr + mcap);
    int* k0 = idx + mcap;
    int* bin = k0 + mcap;
    int* nk = bin + mcap;
    __shared__ int s_m;
    __shared__ double s_voiced;
    const int f = blockIdx.x, tid = threadIdx.x;
    const double* row = cmnd + (int64_t)f * n_lags;
    for (int i = tid; i < n_lags; i += 256) c[i] = row[i];
    for (int i = tid; i < n_bins; i += 256) obs[i] = 0.0;
    __syncthreads();
    if (tid < 64) {                                 // troughs in ascending lag: interior c[i] < c[i-1] && c[i] <= c[i+1], and the two edge rules
        int m = 0;
        for (int base = 0; base < n_lags; base += 64) {
            const int i = base + tid;
            bool tr = false;
            if (i < n_lags) {
                if (i == 0) tr = c[0] < c[1];
                else if (i == n_lags - 1) tr = c[i] < c[i - 1];
                else tr = c[i] < c[i - 1] && c[i] <= c[i + 1];
            }
            const unsigned long long b = __ballot(tr);
            const int at = m + __popcll(b & ((1ull << tid) - 1ull));
            if (tr && at < mcap) idx[at] = i;
            m += __popcll(b);
        }
        if (tid == 0) s_m = m < mcap ? m : mcap;
    }
    __syncthreads();
    const int m = s_m;
    for (int i = tid; i < m; i += 256) {
        const int j = idx[i];
        const double hv = c[j];
        h[i] = hv;
        int k = 0;
        while (k < n_thr && !(hv < thr[k])) ++k;
        k0[i] = k;
        double shift = 0.0;                         // parabolic refinement of the lag; 0 at the edges and where |shift| > 1
        if (j > 0 && j < n_lags - 1) {
            const double a = (c[j - 1] + c[j + 1] - 2.0 * c[j]) / 2.0, b = (c[j + 1] - c[j - 1]) / 2.0;
            shift = -b / (2.0 * a + F_TINY);
            if (fabs(shift) > 1.0) shift = 0.0;
        }
        const double period = (double)(min_p + j) + shift;
        double bn = rint(bins_per_octave * log2((pitch_sr / period) / f_min));      // np.round: half to even
        if (!(bn >= 0.0)) bn = 0.0;
        if (bn > (double)n_bins) bn = (double)n_bins;
        bin[i] = (int)bn;
    }
    __syncthreads();
    for (int k = tid; k < n_thr; k += 256) {
        int n = 0;
        for (int i = 0; i < m; ++i) n += k0[i] <= k ? 1 : 0;
        nk[k] = n;
    }
    __syncthreads();
    const double e2 = exp(-2.0);
    for (int i = tid; i < m; i += 256) {            // Boltzmann(2) prior over the troughs below each threshold, Beta mass per threshold
        double p = 0.0;
        for (int k = k0[i]; k < n_thr; ++k) {
            int pos = 0;
            for (int q = 0; q < i; ++q) pos += k0[q] <= k ? 1 : 0;
            const int n = nk[k] > 1 ? nk[k] : 1;
            p += (1.0 - e2) * exp(-2.0 * (double)pos) / (1.0 - exp(-2.0 * (double)n)) * beta[k];
        }
        pr[i] = p;
    }
    __syncthreads();
    if (tid == 0 && m > 0) {
        int g = 0;                                  // the no-trough mass goes to the global minimum (first one), over the thresholds not above it
        for (int i = 1; i < m; ++i) if (h[i] < h[g]) g = i;
        double bs = 0.0;
        for (int k = 0; k < k0[g]; ++k) bs += beta[k];
        pr[g] += no_trough * bs;
        for (int i = 0; i < m; ++i)                 // ascending lag: a later trough in the same bin wins; bin n_bins falls into the unvoiced columns
            if (pr[i] != 0.0 && bin[i] < n_bins) obs[bin[i]] = pr[i];
    }
    __syncthreads();
    if (tid < 64) {
        double v = 0.0;
        for (int i = tid; i < n_bins; i += 64) v += obs[i];
        v = wave_sum_f64(v);
        if (tid == 0) s_voiced = fmin(1.0, fmax(0.0, v));
    }
    __syncthreads();
    const double unv = log((1.0 - s_voiced) / (double)n_bins + F_TINY);
    double* o = out + (int64_t)f * 2 * n_bins;
    for (int i = tid; i < n_bins; i += 256) {
        o[i] = log(obs[i] + F_TINY);
        o[n_bins + i] = unv;
    }
}

// (value, state) of the larger value; equal values: the lower state (np.argmax's first maximum)
__device__ __forceinline__ void vit_take(double& v, int& s, double ov, int os) {
    if (ov > v || (ov == v && os < s)) { v = ov; s = os; }
}

// One clip per workgroup: the Viterbi pass over 2 n_bins states in add-and-compare form.  State values are double-buffered in LDS, one
// barrier per frame; backpointers go to HBM; lane 0 backtracks.  A to-state (v, j) scans its predecessors in ascending state index -
// the voiced block before the unvoiced one, ascending from-bin inside a block - and a candidate replaces the best only on a strict >.
// States outside the band reach it with log(tiny): max(val) + log(tiny), with the first arg-max of val as predecessor, wins wherever
// it beats every candidate inside.  (max, arg-max) of a frame's values are reduced while the values are produced and read by the next
// frame.  Only float64 adds and compares in the host's association: (val[from] + lt), then log_obs + best.
// Dynamic LDS: val[2][S] | wmax[2][16] (doubles) | warg[2][16] (ints).
__global__ __launch_bounds__(1024) void k_feat_viterbi(const double* __restrict__ log_obs, const FeatClip* __restrict__ clips, int n_bins, int hw,
                                                       const double* __restrict__ trans, const double* __restrict__ log_init, double log_tiny,
                                                       int* __restrict__ ptr, int* __restrict__ states, int states_stride) {
    extern __shared__ double vsh[];
    const int S = 2 * n_bins, W = 2 * hw + 1;
    double* val = vsh;
    double* wmax = val + 2 * S;
    int* warg = (int*)(wmax + 32);
    const int clip = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
    const int T = clips[clip].frames;
    const int64_t f0 = clips[clip].first;
    for (int t = 0; t < T; ++t) {
        double* cur = val + (t & 1) * S;
        const double* prev = val + ((t & 1) ^ 1) * S;
        const double* lo = log_obs + (f0 + t) * S;
        double pmax = -INFINITY;
        int parg = INT_MAX;
        if (t > 0)
            for (int w = 0; w < n_waves; ++w) vit_take(pmax, parg, wmax[((t & 1) ^ 1) * 16 + w], warg[((t & 1) ^ 1) * 16 + w]);
        const double out_best = pmax + log_tiny;
        double lbest = -INFINITY;
        int larg = INT_MAX;
        for (int s = tid; s < S; s += blockDim.x) {
            double v;
            if (t == 0) {
                v = lo[s] + log_init[s];
            } else {
                const int v_to = s >= n_bins ? 1 : 0, j = s - v_to * n_bins;
                const int o_lo = -hw > -j ? -hw : -j, o_hi = hw < n_bins - 1 - j ? hw : n_bins - 1 - j;
                double best = -INFINITY;
                int arg = 0;
                for (int v_from = 0; v_from < 2; ++v_from) {
                    const double* tab = trans + ((int64_t)(v_from == v_to ? 0 : 1) * W + (o_lo + hw)) * n_bins + j;
                    const double* pv = prev + v_from * n_bins + j + o_lo;
                    for (int o = o_lo; o <= o_hi; ++o, ++pv, tab += n_bins) {
                        const double cand = *pv + *tab;
                        if (cand > best) { best = cand; arg = v_from * n_bins + j + o; }
                    }
                }
                if (out_best > best) { best = out_best; arg = parg; }
                ptr[(f0 + t) * S + s] = arg;
                v = lo[s] + best;
            }
            cur[s] = v;
            if (v > lbest || larg == INT_MAX) { lbest = v; larg = s; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) vit_take(lbest, larg, __shfl_xor(lbest, o, 64), __shfl_xor(larg, o, 64));
        if (lane == 0) { wmax[(t & 1) * 16 + wave] = lbest; warg[(t & 1) * 16 + wave] = larg; }
        __syncthreads();                            // publishes cur, the wave maxima and (workgroup scope) this frame's backpointers
    }
    int* out = states + (int64_t)clip * states_stride;
    for (int t = T + tid; t < states_stride; t += blockDim.x) out[t] = -1;
    if (tid == 0 && T > 0) {
        double fmax_v = -INFINITY;
        int st = INT_MAX;
        for (int w = 0; w < n_waves; ++w) vit_take(fmax_v, st, wmax[((T - 1) & 1) * 16 + w], warg[((T - 1) & 1) * 16 + w]);
        if (st < 0 || st >= S) st = 0;
        out[T - 1] = st;
        for (int t = T - 2; t >= 0; --t) {
            st = ptr[(f0 + t + 1) * S + st];
            out[t] = st;
        }
    }
}

template <class T>
int feat_grow(rt_ctx* ctx, FeatBuf<T>& b, size_t need) {
    if (need <= b.cap && b.p) return RT_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
    if (need == 0) need = 1;
    RT_HIP(ctx, hipMalloc((void**)&b.p, need * sizeof(T)));
    b.cap = need;
    return RT_OK;
}

// log-obs [n_frames][2 n_bins] of cmnd [n_frames][n_lags], both in HBM, on the context's stream
int feat_observe(rt_features* s, const double* d_cmnd, int n_frames, int n_lags, int min_p, double* d_logobs) {
    const int mcap = (n_lags + 1) / 2 + 1;
    const size_t lds = (size_t)(n_lags + s->pm_bins + 2 * mcap) * 8 + (size_t)(3 * mcap + s->pm_thr) * 4;
    if (lds > 60 * 1024) return rt_fail(s->ctx, RT_ERR_INVALID, "pitch observation stage: %zu bytes of LDS per frame", lds);
    hipLaunchKernelGGL(k_feat_observe, dim3(n_frames), dim3(256), lds, s->ctx->stream, d_cmnd, n_lags, min_p, s->pm_bins, s->pm_thr, s->pm_d_thr,
                       s->pm_d_beta, s->pm_sr, s->pm_fmin, s->pm_bins_per_octave, s->pm_no_trough, d_logobs);
    return RT_OK;
}

// state paths [n_clips][stride] (-1 behind a clip's last frame) of the log-obs of n_clips clips laid back to back; the clip table
// gives every clip's first frame and frame count
int feat_viterbi(rt_features* s, const double* d_logobs, const FeatClip* d_clips, int n_clips, int* d_ptr, int* d_states, int stride) {
    const int S = 2 * s->pm_bins, rounds = (S + 1023) / 1024;
    const int threads = std::min(1024, (((S + rounds - 1) / rounds) + 63) / 64 * 64);
    const size_t lds = (size_t)(2 * S + 32) * 8 + 32 * 4;
    hipLaunchKernelGGL(k_feat_viterbi, dim3(n_clips), dim3(threads), lds, s->ctx->stream, d_logobs, d_clips, s->pm_bins, s->pm_hw, s->pm_d_trans,
                       s->pm_d_init, s->pm_log_tiny, d_ptr, d_states, stride);
    return RT_OK;
}

int feat_tables(rt_features* s) {
    rt_ctx* ctx = s->ctx;
    std::vector<double> c(F_NFFT), sn(F_NFFT);
    for (int i = 0; i < F_NFFT; ++i) { c[i] = std::cos(2.0 * M_PI * i / F_NFFT); sn[i] = std::sin(2.0 * M_PI * i / F_NFFT); }
    // slaney mel scale, slaney normalisation, 0 .. sr / 2 (librosa.filters.mel defaults)
    auto hz2mel = [](double f) { return f >= 1000.0 ? 15.0 + std::log(f / 1000.0) / (std::log(6.4) / 27.0) : f / (200.0 / 3.0); };
    auto mel2hz = [](double m) { return m >= 15.0 ? 1000.0 * std::exp((std::log(6.4) / 27.0) * (m - 15.0)) : (200.0 / 3.0) * m; };
    std::vector<double> mel_f(F_MELS + 2);
    const double m_hi = hz2mel(F_SR / 2.0);
    for (int i = 0; i < F_MELS + 2; ++i) mel_f[i] = mel2hz(m_hi * i / (F_MELS + 1));
    std::vector<float> melT((size_t)F_BINS * F_MELS);
    for (int k = 0; k < F_BINS; ++k) {
        const double fk = (F_SR / 2.0) * k / (F_BINS - 1);
        for (int m = 0; m < F_MELS; ++m) {
            const double lower = (fk - mel_f[m]) / (mel_f[m + 1] - mel_f[m]), upper = (mel_f[m + 2] - fk) / (mel_f[m + 2] - mel_f[m + 1]);
            melT[(size_t)k * F_MELS + m] = (float)(std::max(0.0, std::min(lower, upper)) * (2.0 / (mel_f[m + 2] - mel_f[m])));
        }
    }
    std::vector<double> dct((size_t)F_MFCC * F_MELS);
    for (int k = 0; k < F_MFCC; ++k)
        for (int n = 0; n < F_MELS; ++n)
            dct[(size_t)k * F_MELS + n] = std::cos(M_PI * k * (2 * n + 1) / (2.0 * F_MELS)) * std::sqrt(2.0 / F_MELS) * (k == 0 ? std::sqrt(0.5) : 1.0);
    RT_HIP(ctx, hipMalloc((void**)&s->d_twc, F_NFFT * 8));
    RT_HIP(ctx, hipMalloc((void**)&s->d_tws, F_NFFT * 8));
    RT_HIP(ctx, hipMalloc((void**)&s->d_melT, melT.size() * 4));
    RT_HIP(ctx, hipMalloc((void**)&s->d_dct, dct.size() * 8));
    RT_HIP(ctx, hipMemcpy(s->d_twc, c.data(), F_NFFT * 8, hipMemcpyHostToDevice));
    RT_HIP(ctx, hipMemcpy(s->d_tws, sn.data(), F_NFFT * 8, hipMemcpyHostToDevice));
    RT_HIP(ctx, hipMemcpy(s->d_melT, melT.data(), melT.size() * 4, hipMemcpyHostToDevice));
    RT_HIP(ctx, hipMemcpy(s->d_dct, dct.data(), dct.size() * 8, hipMemcpyHostToDevice));
    return RT_OK;
}

// the clip table of the call (s->h_clips) to the device, on the context's stream
int feat_upload_clips(rt_features* s) {
    RT_TRY(feat_grow(s->ctx, s->clips, s->h_clips.size()));
    RT_HIP(s->ctx, hipMemcpyAsync(s->clips.p, s->h_clips.data(), s->h_clips.size() * sizeof(FeatClip), hipMemcpyHostToDevice, s->ctx->stream));
    return RT_OK;
}

// The one extraction path: the front half of n_clips clips - one launch per stage - and, with states_stride > 0, pYIN's back half.
// It leaves stats [clips][26], lpc [clips][order + 1], cmnd [frames][lags] (want_cmnd) and the state paths [clips][states_stride] in the
// workspaces and every clip's frame count in s->h_clips, enqueued on the context's stream: the caller copies out what it returns and
// synchronises.  A clip of more than cap_frames frames ends the call with cap_status, as every refusal does before anything is launched.
int feat_run(rt_features* s, const char* who, const float* const* d_pcm, const int64_t* n_samples, int n_clips, int sr_in, int min_p, int max_p, int order,
             bool want_cmnd, int states_stride, int cap_frames, int cap_status) {
    rt_ctx* ctx = s->ctx;
    const bool resample = sr_in != F_SR, want_states = states_stride > 0;
    if (resample) RT_TRY(resampler_design(ctx, s->rs, sr_in, F_SR));
    if (n_clips > 65535) return rt_fail(ctx, RT_ERR_INVALID, "%s: more than 65535 clips in one call", who);      // (the clip is a grid's y)
    s->h_clips.assign((size_t)n_clips, FeatClip{});
    int64_t pcm_total = 0, frames_total = 0, max16 = 0, max_frames = 0;
    for (int c = 0; c < n_clips; ++c) {
        FeatClip& h = s->h_clips[c];
        if (!d_pcm[c] || n_samples[c] < 2) return rt_fail(ctx, RT_ERR_INVALID, "%s: clip %d has fewer than two samples", who, c);
        h.pcm_in = d_pcm[c];
        h.n_in = n_samples[c];
        h.n16 = resample ? s->rs.n_out(h.n_in) : h.n_in;
        if (h.n16 < 2) return rt_fail(ctx, RT_ERR_INVALID, "%s: clip %d has fewer than two samples at 16 kHz", who, c);
        // centre-padded framing: 1 + n // hop frames for both the MFCC and the pitch front end (same frame and hop lengths)
        const int64_t nf = 1 + h.n16 / F_HOP;
        if (nf > cap_frames) return rt_fail(ctx, cap_status, "%s: clip %d has %lld pitch frames, room for %d", who, c, (long long)nf, cap_frames);
        h.first = (int)frames_total;
        h.frames = (int)nf;
        pcm_total += resample ? h.n16 : 0;
        frames_total += nf;
        max16 = std::max(max16, h.n16);
        max_frames = std::max(max_frames, nf);
        if (want_states && frames_total > (int64_t)1 << 20) return rt_fail(ctx, RT_ERR_INVALID, "%s: more than 2^20 frames in one batch", who);
    }
    const int n_lags = max_p - min_p + 1, S = 2 * s->pm_bins;
    const size_t F = (size_t)frames_total;
    if (resample) RT_TRY(feat_grow(ctx, s->pcm, (size_t)pcm_total));
    RT_TRY(feat_grow(ctx, s->logmel, F * F_MELS));
    RT_TRY(feat_grow(ctx, s->mfcc, F * F_MFCC));
    if (want_cmnd) RT_TRY(feat_grow(ctx, s->cmnd, F * n_lags));
    RT_TRY(feat_grow(ctx, s->stats, (size_t)n_clips * 2 * F_MFCC));
    RT_TRY(feat_grow(ctx, s->lpc, (size_t)n_clips * (order + 1)));
    RT_TRY(feat_grow(ctx, s->gmax, (size_t)n_clips));
    if (want_states) {
        RT_TRY(feat_grow(ctx, s->logobs, F * S));
        RT_TRY(feat_grow(ctx, s->ptr, F * S));
        RT_TRY(feat_grow(ctx, s->states, (size_t)n_clips * states_stride));
    }
    int64_t off = 0;
    for (FeatClip& h : s->h_clips) {
        h.pcm16 = resample ? s->pcm.p + off : h.pcm_in;
        off += resample ? h.n16 : 0;
    }
    RT_TRY(feat_upload_clips(s));
    RT_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)s->gmax.p, (int)0x80000000, (size_t)n_clips, ctx->stream));      // below every ordered float
    const dim3 frames((unsigned)max_frames, n_clips);
    if (resample)
        hipLaunchKernelGGL(k_feat_resample, dim3((unsigned)std::min<int64_t>((max16 + 255) / 256, 4096), n_clips), dim3(256), 0, ctx->stream, s->clips.p,
                           s->rs.L, s->rs.M, s->rs.taps, s->rs.half, s->rs.d_h);
    hipLaunchKernelGGL(k_feat_logmel, frames, dim3(256), (size_t)(3 * F_NFFT + F_BINS) * sizeof(double), ctx->stream, s->clips.p, s->d_twc, s->d_tws, s->d_melT,
                       s->logmel.p, s->gmax.p);
    hipLaunchKernelGGL(k_feat_dct, frames, dim3(64), 0, ctx->stream, s->clips.p, s->logmel.p, s->gmax.p, s->d_dct, s->mfcc.p);
    hipLaunchKernelGGL(k_feat_stats, dim3(n_clips, F_MFCC), dim3(64), 0, ctx->stream, s->clips.p, s->mfcc.p, s->stats.p);
    if (want_cmnd) hipLaunchKernelGGL(k_feat_cmnd, frames, dim3(512), 0, ctx->stream, s->clips.p, min_p, max_p, s->cmnd.p);
    hipLaunchKernelGGL(k_feat_lpc, dim3(n_clips), dim3(64), 0, ctx->stream, s->clips.p, order, s->lpc.p);
    RT_HIP(ctx, hipGetLastError());
    if (want_states) {                              // one launch each over every frame / every clip of the call
        RT_TRY(feat_observe(s, s->cmnd.p, (int)F, n_lags, min_p, s->logobs.p));
        RT_TRY(feat_viterbi(s, s->logobs.p, s->clips.p, n_clips, s->ptr.p, s->states.p, states_stride));
        RT_HIP(ctx, hipGetLastError());
    }
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_features_create(rt_ctx* ctx, rt_features** out) {
    if (!ctx || !out) return rt_fail(ctx, RT_ERR_INVALID, "rt_features_create: null argument");
    *out = nullptr;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    rt_features* s = new rt_features();
    s->ctx = ctx;
    const int rc = feat_tables(s);
    if (rc) { delete s; return rc; }
    *out = s;
    return RT_OK;
}

int rt_features_destroy(rt_features* s) {
    if (!s) return RT_OK;
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (void* p : {(void*)s->d_twc, (void*)s->d_tws, (void*)s->d_melT, (void*)s->d_dct, (void*)s->rs.d_h, (void*)s->pm_d_thr, (void*)s->pm_d_beta,
                    (void*)s->pm_d_trans, (void*)s->pm_d_init, (void*)s->pcm.p, (void*)s->logmel.p, (void*)s->mfcc.p, (void*)s->cmnd.p, (void*)s->logobs.p,
                    (void*)s->ptr.p, (void*)s->states.p, (void*)s->stats.p, (void*)s->lpc.p, (void*)s->gmax.p, (void*)s->clips.p})
        if (p) (void)hipFree(p);
    delete s;
    return RT_OK;
}

int rt_features_geometry(int32_t pitch_sr, double fmin, double fmax, int32_t* min_period, int32_t* max_period) {
    if (pitch_sr < 1000 || !(fmin > 0) || !(fmax > fmin) || !min_period || !max_period) return RT_ERR_INVALID;
    *min_period = std::max((int)std::floor(pitch_sr / fmax), 1);
    *max_period = std::min((int)std::ceil(pitch_sr / fmin), P_FRAME - P_WIN - 1);
    return RT_OK;
}

int rt_features_extract(rt_features* s, const float* d_pcm, int64_t n_samples, int32_t sample_rate_in, int32_t min_period, int32_t max_period,
                        int32_t lpc_order, double* h_mfcc_stats26, int32_t* h_n_mfcc_frames, double* h_cmnd, int32_t cmnd_cap_frames,
                        int32_t* h_n_pitch_frames, double* h_lpc) {
    if (!s || !d_pcm || n_samples < 2 || sample_rate_in < 1000 || !h_mfcc_stats26 || !h_n_pitch_frames || !h_lpc || lpc_order < 1 || lpc_order > LPC_MAX ||
        min_period < 1 || max_period <= min_period || max_period > P_FRAME - P_WIN - 1)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_features_extract: bad argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    // one clip, no back half; without h_cmnd the difference function is not computed and any frame count fits
    RT_TRY(feat_run(s, "rt_features_extract", &d_pcm, &n_samples, 1, sample_rate_in, min_period, max_period, lpc_order, h_cmnd != nullptr, 0,
                    h_cmnd ? cmnd_cap_frames : INT_MAX, RT_ERR_LENGTH));
    const int n_frames = s->h_clips[0].frames, n_lags = max_period - min_period + 1;
    RT_HIP(ctx, hipMemcpyAsync(h_mfcc_stats26, s->stats.p, 2 * F_MFCC * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (h_cmnd) RT_HIP(ctx, hipMemcpyAsync(h_cmnd, s->cmnd.p, (size_t)n_frames * n_lags * 8, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipMemcpyAsync(h_lpc, s->lpc.p, (size_t)(lpc_order + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_n_mfcc_frames) *h_n_mfcc_frames = n_frames;
    *h_n_pitch_frames = n_frames;
    return RT_OK;
}

int rt_features_set_pitch_model(rt_features* s, int32_t n_bins, int32_t half_width, int32_t n_thresholds, const double* h_thresholds,
                                const double* h_beta, const double* h_log_trans, const double* h_log_init, double log_tiny, double pitch_sr, double fmin,
                                int32_t bins_per_semitone, double no_trough_prob) {
    if (!s || n_bins < 1 || n_bins > 2000 || half_width < 0 || half_width > 4096 || n_thresholds < 1 || n_thresholds > 1024 || !h_thresholds || !h_beta ||
        !h_log_trans || !h_log_init || !(pitch_sr > 0) || !(fmin > 0) || bins_per_semitone < 1)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_features_set_pitch_model: bad argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    s->pm_set = false;
    for (double** p : {&s->pm_d_thr, &s->pm_d_beta, &s->pm_d_trans, &s->pm_d_init}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    const size_t n_trans = (size_t)2 * (2 * half_width + 1) * n_bins;
    RT_HIP(ctx, hipMalloc((void**)&s->pm_d_thr, (size_t)n_thresholds * 8));
    RT_HIP(ctx, hipMalloc((void**)&s->pm_d_beta, (size_t)n_thresholds * 8));
    RT_HIP(ctx, hipMalloc((void**)&s->pm_d_trans, n_trans * 8));
    RT_HIP(ctx, hipMalloc((void**)&s->pm_d_init, (size_t)2 * n_bins * 8));
    RT_HIP(ctx, hipMemcpy(s->pm_d_thr, h_thresholds, (size_t)n_thresholds * 8, hipMemcpyHostToDevice));
    RT_HIP(ctx, hipMemcpy(s->pm_d_beta, h_beta, (size_t)n_thresholds * 8, hipMemcpyHostToDevice));
    RT_HIP(ctx, hipMemcpy(s->pm_d_trans, h_log_trans, n_trans * 8, hipMemcpyHostToDevice));
    RT_HIP(ctx, hipMemcpy(s->pm_d_init, h_log_init, (size_t)2 * n_bins * 8, hipMemcpyHostToDevice));
    s->pm_bins = n_bins; s->pm_hw = half_width; s->pm_thr = n_thresholds;
    s->pm_log_tiny = log_tiny; s->pm_sr = pitch_sr; s->pm_fmin = fmin; s->pm_bins_per_octave = 12.0 * bins_per_semitone; s->pm_no_trough = no_trough_prob;
    s->pm_set = true;
    return RT_OK;
}

int rt_features_extract_batch(rt_features* s, const float* const* d_pcm, const int64_t* n_samples, int32_t n_clips, int32_t sample_rate_in,
                              int32_t min_period, int32_t max_period, int32_t lpc_order, double* h_mfcc_stats26, double* h_lpc, int32_t* h_states,
                              int32_t cap_frames, int32_t* h_n_pitch_frames) {
    if (!s || !d_pcm || !n_samples || n_clips < 1 || sample_rate_in < 1000 || !h_mfcc_stats26 || !h_lpc || !h_states || !h_n_pitch_frames || lpc_order < 1 ||
        lpc_order > LPC_MAX || min_period < 1 || max_period <= min_period || max_period > P_FRAME - P_WIN - 1 || cap_frames < 1)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_features_extract_batch: bad argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    if (!s->pm_set) return rt_fail(ctx, RT_ERR_INVALID, "rt_features_extract_batch: no pitch model (rt_features_set_pitch_model)");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    RT_TRY(feat_run(s, "rt_features_extract_batch", d_pcm, n_samples, n_clips, sample_rate_in, min_period, max_period, lpc_order, true, cap_frames, cap_frames,
                    RT_ERR_INVALID));
    RT_HIP(ctx, hipMemcpyAsync(h_mfcc_stats26, s->stats.p, (size_t)n_clips * 2 * F_MFCC * 8, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipMemcpyAsync(h_lpc, s->lpc.p, (size_t)n_clips * (lpc_order + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipMemcpyAsync(h_states, s->states.p, (size_t)n_clips * cap_frames * 4, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < n_clips; ++c) h_n_pitch_frames[c] = s->h_clips[c].frames;
    return RT_OK;
}

int rt_debug_features_observe(rt_features* s, const double* h_cmnd, int32_t n_frames, int32_t n_lags, int32_t min_period, double* h_log_obs) {
    if (!s || !h_cmnd || !h_log_obs || n_frames < 1 || n_frames > (1 << 20) || n_lags < 2 || n_lags > P_FRAME - P_WIN - 1 || min_period < 1)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_debug_features_observe: bad argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    if (!s->pm_set) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_features_observe: no pitch model (rt_features_set_pitch_model)");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    const int S = 2 * s->pm_bins;
    RT_TRY(feat_grow(ctx, s->cmnd, (size_t)n_frames * n_lags));
    RT_TRY(feat_grow(ctx, s->logobs, (size_t)n_frames * S));
    RT_HIP(ctx, hipMemcpyAsync(s->cmnd.p, h_cmnd, (size_t)n_frames * n_lags * 8, hipMemcpyHostToDevice, ctx->stream));
    RT_TRY(feat_observe(s, s->cmnd.p, n_frames, n_lags, min_period, s->logobs.p));
    RT_HIP(ctx, hipGetLastError());
    RT_HIP(ctx, hipMemcpyAsync(h_log_obs, s->logobs.p, (size_t)n_frames * S * 8, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

int rt_debug_features_viterbi(rt_features* s, const double* h_log_obs, const int32_t* h_n_frames, int32_t n_clips, int32_t* h_states, int32_t stride) {
    if (!s || !h_log_obs || !h_n_frames || !h_states || n_clips < 1 || stride < 1)
        return rt_fail(s ? s->ctx : nullptr, RT_ERR_INVALID, "rt_debug_features_viterbi: bad argument");
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    if (!s->pm_set) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_features_viterbi: no pitch model (rt_features_set_pitch_model)");
    RT_HIP(ctx, hipSetDevice(ctx->device));
    s->h_clips.assign((size_t)n_clips, FeatClip{});                 // the clip table with null audio: frames alone
    int64_t frames_total = 0;
    for (int c = 0; c < n_clips; ++c) {
        if (h_n_frames[c] < 1 || h_n_frames[c] > stride) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_features_viterbi: clip %d has %d frames, room for %d", c, h_n_frames[c], stride);
        s->h_clips[c].first = (int)frames_total;
        s->h_clips[c].frames = h_n_frames[c];
        frames_total += h_n_frames[c];
        if (frames_total > (int64_t)1 << 20) return rt_fail(ctx, RT_ERR_INVALID, "rt_debug_features_viterbi: more than 2^20 frames");
    }
    const int S = 2 * s->pm_bins, F = (int)frames_total;
    RT_TRY(feat_grow(ctx, s->logobs, (size_t)F * S));
    RT_TRY(feat_grow(ctx, s->ptr, (size_t)F * S));
    RT_TRY(feat_grow(ctx, s->states, (size_t)n_clips * stride));
    RT_TRY(feat_upload_clips(s));
    RT_HIP(ctx, hipMemcpyAsync(s->logobs.p, h_log_obs, (size_t)F * S * 8, hipMemcpyHostToDevice, ctx->stream));
    RT_TRY(feat_viterbi(s, s->logobs.p, s->clips.p, n_clips, s->ptr.p, s->states.p, stride));
    RT_HIP(ctx, hipGetLastError());
    RT_HIP(ctx, hipMemcpyAsync(h_states, s->states.p, (size_t)n_clips * stride * 4, hipMemcpyDeviceToHost, ctx->stream));
    RT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

}  // extern "C"
