// Speed and pitch control of a waveform that already lives in HBM.
// Stands behind BaseTTS._apply_speed_pitch (base_tts.py:618-650), which hands both to torchaudio:
//   speed: functional.resample(audio, int(sr * speed), sr)      sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99
//   pitch: functional.pitch_shift(audio, sr, steps)             STFT (512, hop 128, periodic Hann, reflect-padded centre) -> phase
//          vocoder at rate 2^(-steps / 12) -> inverse STFT (overlap-add over the window envelope) -> resample(int(sr / rate), sr)
//          -> crop / zero-pad to the input length
// The same two algorithms, evaluated in float64 between the float32 PCM that comes in and the float32 PCM that goes out:
//   k_sp_resample  one output sample per thread; the taps h(p, k) = sinc(pi t) cos^2(pi t / 12) base / o, t = (k - width) base / o -
//                  p base / n, come from this closed form (torchaudio materialises them as a [n][o + 2 width] bank: 726 MB for +4
//                  semitones at 24 kHz, whose reduced rates are 15119 : 12000) and are summed in ascending k
//   k_sp_stft      one frame per workgroup: direct 512-point transform from a twiddle table (as k_logmel_frames_group), magnitude and
//                  angle of the 257 bins, two zero frames behind the last
//   k_sp_vocoder   one wave per bin: each lane sums the wrapped phase increments of a contiguous run of output frames, the run
//                  totals are scanned across the wave, a second pass writes mag (cos, sin) - float64 prefix sums, no atomics
//   k_sp_synth     inverse real transform times the window, one output frame per workgroup
//   k_sp_ola       one thread per stretched sample gathers its <= 4 frames in ascending order and divides by the envelope of the same
//                  frames (a gather: no scatter-add, no atomics)
// Every integer decision - reduced rates, filter half-width, every length - is the host's (rt_speedpitch_plan, built by
// rho_tts_amd/speedpitch.py with torchaudio's own Python expressions); the device decides nothing, so a call copies nothing back and
// waits for nothing.  Nothing here is on the hot path of generation: the kernels are the simple forms.
// PARITY UNPINNED (torchaudio absent): the definition is tests/speed_pitch_ref.py, torchaudio 2.x's algorithm in exact arithmetic.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"

struct rt_speedpitch {
    rt_ctx* ctx = nullptr;
    double *d_twc = nullptr, *d_tws = nullptr;     // cos / sin(2 pi i / 512), built once
    // workspaces, grow-only
    double* mid = nullptr;                         // the speed stage's output when the pitch stage follows
    double *mag = nullptr, *ang = nullptr;         // [257][nf + 2]
    double* spec = nullptr;                        // [n_out][257] (re, im)
    double* frames = nullptr;                      // [n_out][512]
    double* stretch = nullptr;                     // [ls]
    size_t mid_cap = 0, mag_cap = 0, ang_cap = 0, spec_cap = 0, frames_cap = 0, stretch_cap = 0;
};

namespace {

constexpr int SP_NFFT = 512, SP_HOP = 128, SP_BINS = SP_NFFT / 2 + 1;
constexpr double SP_WIDTH = 6.0, SP_ROLLOFF = 0.99;
constexpr int64_t SP_MAX_SAMPLES = (int64_t)1 << 30, SP_MAX_TERM = (int64_t)1 << 30;

// y[i], i < n_valid: sum over k of h(i mod n, k) x[(i div n) o + k - width], x zero outside [0, n_in); zeros up to n_write.
// kk = k - width runs over [c - width, c + width + 1], c = floor(o p / n): |t| >= 6 outside (width >= 6 o / base).
template <class TI, class TO>
__global__ __launch_bounds__(256) void k_sp_resample(const TI* __restrict__ x, int64_t n_in, TO* __restrict__ y, int64_t n_write, int64_t n_valid,
                                                     int64_t o, int64_t n, int64_t width) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_write) return;
    if (i >= n_valid) { y[i] = (TO)0; return; }
    const double base = (double)(o < n ? o : n) * SP_ROLLOFF, scale = base / (double)o;
    const int64_t p = i % n, j = i / n, c = (o * p) / n;
    const double tp = -(double)p / (double)n;
    double acc = 0.0;
    for (int64_t kk = c - width; kk <= c + width + 1 && kk < width + o; ++kk) {
        const double t = (tp + (double)kk / (double)o) * base;
        const int64_t src = j * o + kk;
        if (fabs(t) < SP_WIDTH && src >= 0 && src < n_in) {
            const double a = M_PI * t, w = cos(a / (2.0 * SP_WIDTH));
            const double s = t == 0.0 ? 1.0 : sin(a) / a;
            acc += s * (w * w) * scale * (double)x[src];
        }
    }
    y[i] = (TO)acc;
}

template <class TI, class TO>
__global__ __launch_bounds__(256) void k_sp_copy(const TI* __restrict__ x, int64_t n_in, TO* __restrict__ y, int64_t n_write) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_write) y[i] = i < n_in ? (TO)x[i] : (TO)0;
}

// Frame f = samples [128 f - 256, 128 f + 256) of x, reflected at both ends (L >= 257), times the periodic Hann window; bin b on
// thread b (direct form, twiddle index b i mod 512), the Nyquist bin as an alternating sum over the workgroup.  Frames nf, nf + 1: zeros.
template <class TI>
__global__ __launch_bounds__(256) void k_sp_stft(const TI* __restrict__ x, int64_t L, int nf, const double* __restrict__ twc, const double* __restrict__ tws,
                                                 double* __restrict__ mag, double* __restrict__ ang) {
    __shared__ double xw[SP_NFFT], tc[SP_NFFT], ts[SP_NFFT], part[4];
    const int f = blockIdx.x, tid = threadIdx.x, fs = nf + 2;
    if (f >= nf) {
        for (int b = tid; b < SP_BINS; b += 256) { mag[(int64_t)b * fs + f] = 0.0; ang[(int64_t)b * fs + f] = 0.0; }
        return;
    }
    for (int i = tid; i < SP_NFFT; i += 256) {
        int64_t idx = (int64_t)f * SP_HOP - SP_NFFT / 2 + i;
        if (idx < 0) idx = -idx;
        if (idx >= L) idx = 2 * (L - 1) - idx;
        idx = idx < 0 ? 0 : (idx >= L ? L - 1 : idx);
        tc[i] = twc[i];
        ts[i] = tws[i];
        xw[i] = (double)x[idx] * (0.5 - 0.5 * tc[i]);
    }
    __syncthreads();
    double re = 0.0, im = 0.0;
    int idx = 0;
    for (int i = 0; i < SP_NFFT; ++i) {
        re += xw[i] * tc[idx];
        im -= xw[i] * ts[idx];
        idx = (idx + tid) & (SP_NFFT - 1);
    }
    mag[(int64_t)tid * fs + f] = hypot(re, im);
    ang[(int64_t)tid * fs + f] = atan2(im, re);
    const double alt = wave_sum_f64((tid & 1) ? -(xw[tid] + xw[tid + 256]) : (xw[tid] + xw[tid + 256]));
    if ((tid & 63) == 0) part[tid >> 6] = alt;
    __syncthreads();
    if (tid == 0) {
        const double ny = (part[0] + part[1]) + (part[2] + part[3]);
        mag[(int64_t)(SP_BINS - 1) * fs + f] = fabs(ny);
        ang[(int64_t)(SP_BINS - 1) * fs + f] = atan2(0.0, ny);
    }
}

// Output frame i of bin b: ts = i rate, f0 = floor(ts), alpha = ts - f0; magnitude alpha |S[f0 + 1]| + (1 - alpha) |S[f0]|; phase =
// angle(S[0]) + the sum over the frames before i of the increments d = angle(S[f0 + 1]) - angle(S[f0]) - pa, wrapped to [-pi, pi], + pa
// (pa = b pi 128 / 256).  One wave per bin; lane l owns frames [l R, (l + 1) R).
__device__ __forceinline__ double sp_increment(const double* __restrict__ m, const double* __restrict__ a, int nf, int64_t i, double rate, double pa,
                                               double* mag_out) {
    const double ts = (double)i * rate, fl = floor(ts);
    int64_t f0 = (int64_t)fl;
    if (f0 > nf) f0 = nf;                                                          // (never taken for a consistent plan: i rate < nf)
    const double alpha = ts - fl;
    *mag_out = alpha * m[f0 + 1] + (1.0 - alpha) * m[f0];
    double d = a[f0 + 1] - a[f0] - pa;
    d = d - 2.0 * M_PI * rint(d / (2.0 * M_PI));
    return d + pa;
}

__global__ __launch_bounds__(64) void k_sp_vocoder(const double* __restrict__ mag, const double* __restrict__ ang, int nf, int n_out, double rate,
                                                   double* __restrict__ spec) {
    const int b = blockIdx.x, lane = threadIdx.x, fs = nf + 2;
    const double* m = mag + (int64_t)b * fs;
    const double* a = ang + (int64_t)b * fs;
    const double pa = (double)b * (M_PI * SP_HOP / (SP_BINS - 1));
    const int R = (n_out + 63) / 64;
    const int lo = min(lane * R, n_out), hi = min(lo + R, n_out);
    double run = 0.0, mg;
    for (int i = lo; i < hi; ++i) run += sp_increment(m, a, nf, i, rate, pa, &mg);
    double incl = run;                                                             // inclusive scan of the run totals
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const double up = __shfl_up(incl, s, 64);
        if (lane >= s) incl += up;
    }
    const double before = __shfl_up(incl, 1, 64);
    double phase = a[0] + (lane == 0 ? 0.0 : before);
    for (int i = lo; i < hi; ++i) {
        const double d = sp_increment(m, a, nf, i, rate, pa, &mg);
        double sn, cs;
        sincos(phase, &sn, &cs);
        spec[((int64_t)i * SP_BINS + b) * 2] = mg * cs;
        spec[((int64_t)i * SP_BINS + b) * 2 + 1] = mg * sn;
        phase += d;
    }
}

// frames[f][t] = w[t] / 512 (Re Z0 + (-1)^t Re Z256 + 2 sum_{b = 1..255} (Re Zb cos(2 pi b t / 512) - Im Zb sin(2 pi b t / 512)))
__global__ __launch_bounds__(256) void k_sp_synth(const double* __restrict__ spec, const double* __restrict__ twc, const double* __restrict__ tws,
                                                  double* __restrict__ frames) {
    __shared__ double zr[SP_BINS], zi[SP_BINS], tc[SP_NFFT], ts[SP_NFFT];
    const int f = blockIdx.x, tid = threadIdx.x;
    for (int b = tid; b < SP_BINS; b += 256) {
        zr[b] = spec[((int64_t)f * SP_BINS + b) * 2];
        zi[b] = spec[((int64_t)f * SP_BINS + b) * 2 + 1];
    }
    for (int i = tid; i < SP_NFFT; i += 256) { tc[i] = twc[i]; ts[i] = tws[i]; }
    __syncthreads();
    for (int t = tid; t < SP_NFFT; t += 256) {
        double acc = 0.0;
        int idx = t;
        for (int b = 1; b < SP_BINS - 1; ++b) {
            acc += zr[b] * tc[idx] - zi[b] * ts[idx];
            idx = (idx + t) & (SP_NFFT - 1);
        }
        const double v = (zr[0] + ((t & 1) ? -zr[SP_BINS - 1] : zr[SP_BINS - 1])) + 2.0 * acc;
        frames[(int64_t)f * SP_NFFT + t] = v / SP_NFFT * (0.5 - 0.5 * tc[t]);
    }
}

// stretched sample s = position q = s + 256 of the overlap-add: the frames that cover q in ascending order over the sum of their
// squared windows; zero behind the last frame's end
__global__ __launch_bounds__(256) void k_sp_ola(const double* __restrict__ frames, const double* __restrict__ twc, int n_out, int64_t ls,
                                                double* __restrict__ stretch) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= ls) return;
    const int64_t q = s + SP_NFFT / 2, total = SP_NFFT + (int64_t)SP_HOP * (n_out - 1);
    if (q >= total) { stretch[s] = 0.0; return; }
    const int64_t f_lo = q < SP_NFFT ? 0 : (q - SP_NFFT) / SP_HOP + 1, f_hi = std::min<int64_t>(n_out - 1, q / SP_HOP);
    double acc = 0.0, env = 0.0;
    for (int64_t f = f_lo; f <= f_hi; ++f) {
        const int off = (int)(q - f * SP_HOP);
        const double w = 0.5 - 0.5 * twc[off];
        acc += frames[f * SP_NFFT + off];
        env += w * w;
    }
    stretch[s] = acc / env;
}

template <class T>
int sp_grow(rt_ctx* ctx, T*& p, size_t& cap, size_t need) {
    if (need <= cap && p) return RT_OK;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    if (need == 0) need = 1;
    RT_HIP(ctx, hipMalloc((void**)&p, need * sizeof(T)));
    cap = need;
    return RT_OK;
}

int64_t sp_gcd(int64_t a, int64_t b) {
    while (b) { const int64_t t = a % b; a = b; b = t; }
    return a;
}

// The terms of one resampler call against what integer arithmetic says about them: coprime rates, width = ceil(6 o / (0.99 min(o, n)))
// (the host rounds a float quotient up: one more than the exact ceiling is accepted, it only adds taps that are zero), output
// length ceil(n len / o).  o == n: the call copies.
bool sp_resample_ok(int64_t o, int64_t n, int64_t width, int64_t len_in, int64_t len_out) {
    if (o < 1 || n < 1 || o > SP_MAX_TERM || n > SP_MAX_TERM || len_in < 0 || len_in > SP_MAX_SAMPLES) return false;
    if (o == n) return len_out == len_in;
    if (sp_gcd(o, n) != 1) return false;
    const int64_t m = std::min(o, n), exact = (600 * o + 99 * m - 1) / (99 * m);
    if (width < exact || width > exact + 1) return false;
    const __int128 num = (__int128)n * len_in + o - 1;
    return (__int128)len_out == num / o && len_out <= SP_MAX_SAMPLES;
}

inline unsigned sp_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + 255) / 256); }

template <class TI, class TO>
void sp_launch_resample(hipStream_t st, const TI* x, int64_t n_in, TO* y, int64_t n_write, int64_t n_valid, int64_t o, int64_t n, int64_t width) {
    if (n_write <= 0) return;
    if (o == n) hipLaunchKernelGGL((k_sp_copy<TI, TO>), dim3(sp_blocks(n_write)), dim3(256), 0, st, x, std::min(n_in, n_valid), y, n_write);
    else hipLaunchKernelGGL((k_sp_resample<TI, TO>), dim3(sp_blocks(n_write)), dim3(256), 0, st, x, n_in, y, n_write, n_valid, o, n, width);
}

}  // namespace

extern "C" {

int rt_speedpitch_create(rt_ctx* ctx, rt_speedpitch** out) {
    if (!ctx || !out) return rt_fail(ctx, RT_ERR_INVALID, "rt_speedpitch_create: null argument");
    *out = nullptr;
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<double> c(SP_NFFT), sn(SP_NFFT);
    for (int i = 0; i < SP_NFFT; ++i) { c[i] = std::cos(2.0 * M_PI * i / SP_NFFT); sn[i] = std::sin(2.0 * M_PI * i / SP_NFFT); }
    rt_speedpitch* s = new rt_speedpitch();
    s->ctx = ctx;
    hipError_t e = hipMalloc((void**)&s->d_twc, SP_NFFT * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&s->d_tws, SP_NFFT * 8);
    if (e == hipSuccess) e = hipMemcpy(s->d_twc, c.data(), SP_NFFT * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_tws, sn.data(), SP_NFFT * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (s->d_twc) (void)hipFree(s->d_twc);
        if (s->d_tws) (void)hipFree(s->d_tws);
        delete s;
        return rt_fail(ctx, rt_hip_status(e), "%srt_speedpitch_create: %s", e == hipErrorOutOfMemory ? "out of memory: " : "", hipGetErrorString(e));
    }
    *out = s;
    return RT_OK;
}

int rt_speedpitch_destroy(rt_speedpitch* s) {
    if (!s) return RT_OK;
    rt_ctx* ctx = s->ctx;
    CtxLock g(ctx);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (void* p : {(void*)s->d_twc, (void*)s->d_tws, (void*)s->mid, (void*)s->mag, (void*)s->ang, (void*)s->spec, (void*)s->frames, (void*)s->stretch})
        if (p) (void)hipFree(p);
    delete s;
    return RT_OK;
}

int rt_speedpitch_apply(rt_speedpitch* s, const float* d_in, int64_t n_in, const rt_speedpitch_plan* p, float* d_out, int64_t out_capacity) {
    if (!s) return RT_ERR_INVALID;
    rt_ctx* ctx = s->ctx;
    if (!d_in || !p || !d_out || n_in < 1 || n_in > SP_MAX_SAMPLES) return rt_fail(ctx, RT_ERR_INVALID, "rt_speedpitch_apply: bad argument");
    const bool speed = p->do_speed != 0, pitch = p->do_pitch != 0;
    if (!speed && !pitch) return rt_fail(ctx, RT_ERR_INVALID, "rt_speedpitch_apply: the plan runs neither stage");
    if (speed && !sp_resample_ok(p->s_o, p->s_n, p->s_width, n_in, p->s_len))
        return rt_fail(ctx, RT_ERR_INVALID, "rt_speedpitch_apply: speed stage %lld : %lld, width %lld, %lld -> %lld samples is inconsistent", (long long)p->s_o,
                       (long long)p->s_n, (long long)p->s_width, (long long)n_in, (long long)p->s_len);
    const int64_t L = speed ? p->s_len : n_in;
    if (p->L != L || L < 1) return rt_fail(ctx, RT_ERR_INVALID, "rt_speedpitch_apply: plan says %lld samples, the stages give %lld", (long long)p->L, (long long)L);
    if (pitch) {
        const double rate = p->rate;
        if (L <= SP_NFFT / 2) return rt_fail(ctx, RT_ERR_INVALID, "rt_speedpitch_apply: the pitch stage needs more than %d samples, got %lld", SP_NFFT / 2, (long long)L);
        if (!(rate > 0.0) || !std::isfinite(rate) || p->nf != 1 + L / SP_HOP || p->n_out < 1 || p->n_out > ((int64_t)1 << 24) || p->ls < 1 ||
            p->ls > SP_MAX_SAMPLES || std::fabs((double)p->n_out - (double)p->nf / rate) > 1.0 + 1e-9 * (double)p->n_out ||
            std::fabs((double)p->ls - (double)L / rate) > 1.0 + 1e-9 * (double)p->ls || !sp_resample_ok(p->p_o, p->p_n, p->p_width, p->ls, p->p_len))
            return rt_fail(ctx, RT_ERR_INVALID, "rt_speedpitch_apply: pitch stage (rate %g, %lld frames -> %lld, %lld stretched samples, %lld : %lld width %lld -> %lld) is inconsistent",
                           rate, (long long)p->nf, (long long)p->n_out, (long long)p->ls, (long long)p->p_o, (long long)p->p_n, (long long)p->p_width, (long long)p->p_len);
    }
    if (out_capacity < L) return rt_fail(ctx, RT_ERR_INVALID, "rt_speedpitch_apply: %lld samples, room for %lld", (long long)L, (long long)out_capacity);
    CtxLock g(ctx);
    RT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (!pitch) {
        sp_launch_resample<float, float>(st, d_in, n_in, d_out, L, L, p->s_o, p->s_n, p->s_width);
        RT_HIP(ctx, hipGetLastError());
        return RT_OK;
    }
    const int nf = (int)p->nf, n_out = (int)p->n_out;
    if (speed) RT_TRY(sp_grow(ctx, s->mid, s->mid_cap, (size_t)L));
    RT_TRY(sp_grow(ctx, s->mag, s->mag_cap, (size_t)SP_BINS * (nf + 2)));
    RT_TRY(sp_grow(ctx, s->ang, s->ang_cap, (size_t)SP_BINS * (nf + 2)));
    RT_TRY(sp_grow(ctx, s->spec, s->spec_cap, (size_t)n_out * SP_BINS * 2));
    RT_TRY(sp_grow(ctx, s->frames, s->frames_cap, (size_t)n_out * SP_NFFT));
    RT_TRY(sp_grow(ctx, s->stretch, s->stretch_cap, (size_t)p->ls));
    if (speed) {
        sp_launch_resample<float, double>(st, d_in, n_in, s->mid, L, L, p->s_o, p->s_n, p->s_width);
        hipLaunchKernelGGL(k_sp_stft<double>, dim3(nf + 2), dim3(256), 0, st, s->mid, L, nf, s->d_twc, s->d_tws, s->mag, s->ang);
    } else {
        hipLaunchKernelGGL(k_sp_stft<float>, dim3(nf + 2), dim3(256), 0, st, d_in, L, nf, s->d_twc, s->d_tws, s->mag, s->ang);
    }
    hipLaunchKernelGGL(k_sp_vocoder, dim3(SP_BINS), dim3(64), 0, st, s->mag, s->ang, nf, n_out, p->rate, s->spec);
    hipLaunchKernelGGL(k_sp_synth, dim3(n_out), dim3(256), 0, st, s->spec, s->d_twc, s->d_tws, s->frames);
    hipLaunchKernelGGL(k_sp_ola, dim3(sp_blocks(p->ls)), dim3(256), 0, st, s->frames, s->d_twc, n_out, p->ls, s->stretch);
    sp_launch_resample<double, float>(st, s->stretch, p->ls, d_out, L, std::min(L, p->p_len), p->p_o, p->p_n, p->p_width);
    RT_HIP(ctx, hipGetLastError());
    return RT_OK;
}

}  // extern "C"
