// The windowed-sinc polyphase resampler that brings PCM to 16 kHz for the speech-to-text front end (stt.hip) and the drift features
// (features.hip): one filter design and one tap loop, defined once.  It stays a header on purpose: features.hip is compiled with
// -ffp-contract=off and stt.hip at the compiler's default, so the tap loop's multiply-add may be contracted in one and not in the
// other; inlined into each file's own kernel it keeps that file's bits, where one shared kernel would change one side's.
// (The speed / pitch resampler, speedpitch.hip k_sp_resample, evaluates torchaudio's taps on the fly and is a different function.)
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"

// y[n] = sum_j x[base(n) + j - half] h[phase(n)][j]: sr_in / sr_out = M / L in lowest terms, base = floor(n M / L),
// phase = (n M) mod L; samples outside [0, n_in) are zero.  float64 accumulation in tap order.
__device__ __forceinline__ float resample_at(const float* __restrict__ x, int64_t n_in, int64_t n, int L, int M, int taps, int half,
                                             const float* __restrict__ h) {
    const int64_t num = n * M;
    const int64_t base = num / L;
    const int phase = (int)(num % L);
    const float* hp = h + (int64_t)phase * taps;
    double acc = 0.0;
    for (int j = 0; j < taps; ++j) {
        const int64_t t = base + j - half;
        if (t >= 0 && t < n_in) acc += (double)x[t] * (double)hp[j];
    }
    return (float)acc;
}

// The filter of the last (sr_in -> sr_out) pair a handle was asked for; the owner frees d_h.
struct Resampler {
    float* d_h = nullptr;            // [L][taps] float32
    int sr_in = 0, sr_out = 0, L = 0, M = 0, taps = 0, half = 0;
    int64_t n_out(int64_t n_in) const { return (n_in * L + M - 1) / M; }
};

// Hann window over `width` zero crossings of the low-pass at rolloff x the lower Nyquist: the definition rho_tts_amd/stt.py restates
// in NumPy for the tests (oracle: parity unpinned - the reference's pipeline decodes its temporary WAV through ffmpeg)
inline int resampler_design(rt_ctx* ctx, Resampler& r, int sr_in, int sr_out) {
    if (r.sr_in == sr_in && r.sr_out == sr_out && r.d_h) return RT_OK;
    int a = sr_in, b = sr_out;
    while (b) { const int t = a % b; a = b; b = t; }
    const int L = sr_out / a, M = sr_in / a;
    const double width = 6.0, rolloff = 0.99;
    const double base = std::min(sr_in, sr_out) * rolloff;          // cut-off (both sides) in Hz x 2
    const int half = (int)std::ceil(width * sr_in / base);
    const int taps = 2 * half + 1;
    std::vector<float> h((size_t)L * taps);
    for (int p = 0; p < L; ++p)
        for (int j = 0; j < taps; ++j) {
            // time (in input samples) from tap j of phase p to the output instant: t = (j - half) - p / L
            const double t = ((double)(j - half) - (double)p / L) * base / sr_in;
            double v = 0.0;
            if (std::fabs(t) < width) {
                const double w = std::cos(t * M_PI / width / 2.0);
                const double sinc = t == 0.0 ? 1.0 : std::sin(M_PI * t) / (M_PI * t);
                v = sinc * w * w * base / sr_in;
            }
            h[(size_t)p * taps + j] = (float)v;
        }
    if (r.d_h) (void)hipFree(r.d_h);
    r.d_h = nullptr;
    RT_HIP(ctx, hipMalloc((void**)&r.d_h, h.size() * 4));
    RT_HIP(ctx, hipMemcpy(r.d_h, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    r.sr_in = sr_in; r.sr_out = sr_out; r.L = L; r.M = M; r.taps = taps; r.half = half;
    return RT_OK;
}
