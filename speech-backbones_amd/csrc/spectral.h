// spectral.h -- what the audio kernels share (mel.hip, fgl.hip, wav.hip; internal header): the wave-local Stockham FFT with its LDS
// helpers, the real-spectrum split of a packed transform and the reflect-pad index on the device; the float64 tables (periodic Hann
// window, twiddles, slaney mel filterbank and its rows' contiguous supports) on the host.  One definition each.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

namespace gtts {

// ---------------------------------------------------------------------------------------------------------------------------- device

__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// Orders the LDS traffic of ONE wave: a wave's LDS instructions execute in issue order, so a value written by one lane is there for
// any lane of the same wave that reads it later; this only keeps the compiler from moving accesses across the point.  The waves of a
// workgroup transform their frames without waiting for one another.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Where point j of a transform buffer lives.  The radix-4 passes with stride 1 and 4 store with 16 consecutive lanes 4 and 16 points
// apart: on the 32 banks of a ds_write_b64 lane group that is a 4-way conflict.  XOR-ing bits 4-5 of j into bits 0-1 and 2-3 spreads
// both patterns over all banks and keeps contiguous runs of 16 points contiguous (a permutation inside each run).
__device__ __forceinline__ int fft_at(int j) { return j ^ (5 * ((j >> 4) & 3)); }

// Stockham autosort FFT of M = 2^(LOGN-1) points (decimation in frequency, radix-4 passes and one radix-2 pass when LOGN - 1 is odd)
// by ONE wave between its two bank-swizzled LDS buffers; on return x holds the transform in natural order and y is free.
// tw(pass, r, ps, m), m = 1, 2, 3: the twiddle e^{-2 pi i m ps / M} of the lane's butterfly lane + 64 r in radix-4 pass `pass`
// (ps = p s, its index in the M-point table).  The caller chooses where the twiddles live, with no branch here: mel.hip holds the
// lane's pass twiddles in registers (they are the same for every frame), fgl.hip reads tw[m * ps] from the table in LDS.
template <int LOGN, typename TW>
__device__ __forceinline__ void stockham_fft(float2 *&x, float2 *&y, TW tw, int lane) {
    constexpr int M = 1 << (LOGN - 1), Q = M / 4, RB = (Q + 63) / 64;
    int s = 1, pass = 0;
#pragma unroll
    for (int n = M; n >= 4; n >>= 2, ++pass) {        // sub-transform length n, stride s = M / n
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int i = lane + 64 * r;              // butterfly i = q + s p
            if (Q >= 64 || i < Q) {
                const int q = i & (s - 1), ps = i - q;
                const float2 v0 = x[fft_at(i)], v1 = x[fft_at(i + Q)], v2 = x[fft_at(i + 2 * Q)], v3 = x[fft_at(i + 3 * Q)];
                const float2 apc = make_float2(v0.x + v2.x, v0.y + v2.y), amc = make_float2(v0.x - v2.x, v0.y - v2.y);
                const float2 bpd = make_float2(v1.x + v3.x, v1.y + v3.y);
                const float2 jbmd = make_float2(-(v1.y - v3.y), v1.x - v3.x);        // i (b - d)
                const int o = q + 4 * ps;
                y[fft_at(o)] = make_float2(apc.x + bpd.x, apc.y + bpd.y);
                y[fft_at(o + s)] = cmul(make_float2(amc.x - jbmd.x, amc.y - jbmd.y), tw(pass, r, ps, 1));
                y[fft_at(o + 2 * s)] = cmul(make_float2(apc.x - bpd.x, apc.y - bpd.y), tw(pass, r, ps, 2));
                y[fft_at(o + 3 * s)] = cmul(make_float2(amc.x + jbmd.x, amc.y + jbmd.y), tw(pass, r, ps, 3));
            }
        }
        wave_lds_sync();
        float2 *tmp = x; x = y; y = tmp;
        s <<= 2;
    }
    if ((LOGN - 1) & 1) {                 // the remaining length-2 transforms (s = M / 2)
#pragma unroll
        for (int r = 0; r < (M / 2 + 63) / 64; ++r) {
            const int q = lane + 64 * r;
            const float2 v0 = x[fft_at(q)], v1 = x[fft_at(q + M / 2)];
            y[fft_at(q)] = make_float2(v0.x + v1.x, v0.y + v1.y);
            y[fft_at(q + M / 2)] = make_float2(v0.x - v1.x, v0.y - v1.y);
        }
        wave_lds_sync();
        float2 *tmp = x; x = y; y = tmp;
    }
}

// Bins k and M - k of the real spectrum of 2 M samples packed as M complex points z[m] = x[2m] + i x[2m+1], from Z[k], Z[M-k] and
// W^k = e^{-2 pi i k / (2 M)}:  E = (Z[k] + conj Z[M-k]) / 2,  O = -i (Z[k] - conj Z[M-k]) / 2,  X[k] = E + W^k O,
// X[M-k] = conj(E - W^k O).  Returns E and W^k O.
struct RealSplit { float2 e, wo; };
__device__ __forceinline__ RealSplit real_split(float2 zk, float2 zm, float2 w) {
    const float er = 0.5f * (zk.x + zm.x), ei = 0.5f * (zk.y - zm.y);
    const float orr = 0.5f * (zk.y + zm.y), oi = -0.5f * (zk.x - zm.x);
    return {make_float2(er, ei), make_float2(w.x * orr - w.y * oi, w.x * oi + w.y * orr)};
}

// index j of a row of `len` samples reflected about the row's ends (no edge repeated); one reflection per end: -len < j < 2 len - 1
__device__ __forceinline__ int reflect_index(int j, int len) {
    j = j < 0 ? -j : j;
    return j >= len ? 2 * (len - 1) - j : j;
}

// ------------------------------------------------------------------------------------------------------------------ host, float64

constexpr double TWO_PI = 6.283185307179586476925286766559;

// sample n of the periodic Hann window of `size` samples
inline double hann_periodic(int n, int size) { return 0.5 - 0.5 * std::cos(TWO_PI * n / size); }

// tw[k] = e^{-2 pi i k / period} as (cos, -sin), k < count, rounded to fp32
inline void fill_twiddles(float *tw, int count, int period) {
    for (int k = 0; k < count; ++k) { tw[2 * k] = (float)std::cos(TWO_PI * k / period); tw[2 * k + 1] = (float)-std::sin(TWO_PI * k / period); }
}

// slaney mel scale (librosa htk = False): linear below 1000 Hz, logarithmic above
inline double hz_to_mel(double f) { return f < 1000.0 ? f / (200.0 / 3.0) : 15.0 + std::log(f / 1000.0) / (std::log(6.4) / 27.0); }
inline double mel_to_hz(double m) { return m < 15.0 ? m * (200.0 / 3.0) : 1000.0 * std::exp((std::log(6.4) / 27.0) * (m - 15.0)); }

// librosa.filters.mel with its defaults (slaney scale, slaney area normalisation) in float64, rounded to fp32: fb [nm][n_fft / 2 + 1].
// Edges and bin frequencies are formed as numpy.linspace forms them.
inline void slaney_filterbank(int sampling_rate, int n_fft, int nm, double fmin, double fmax, std::vector<float> &fb) {
    const int nb = n_fft / 2 + 1;
    std::vector<double> f(nm + 2);
    const double lo = hz_to_mel(fmin), hi = hz_to_mel(fmax), step = (hi - lo) / (nm + 1);
    for (int j = 0; j < nm + 2; ++j) f[j] = mel_to_hz(j == nm + 1 ? hi : lo + step * j);
    const double fstep = (0.5 * sampling_rate) / (nb - 1);
    fb.assign((size_t)nm * nb, 0.f);
    for (int i = 0; i < nm; ++i)
        for (int k = 0; k < nb; ++k) {
            const double fk = k == nb - 1 ? 0.5 * sampling_rate : fstep * k;
            const double lower = (fk - f[i]) / (f[i + 1] - f[i]), upper = (f[i + 2] - fk) / (f[i + 2] - f[i + 1]);
            const double w = std::fmax(0.0, std::fmin(lower, upper)) * (2.0 / (f[i + 2] - f[i]));
            fb[(size_t)i * nb + k] = (float)w;
        }
}

// Every filter's support is a contiguous bin range [k0, k1): rows[i] = {k0, chunks, offset into wts, 0}, wts the rows' weights, each
// row zero-padded to whole chunks of `chunk` (1: no padding, rows[i].y counts bins).  An empty filter has no chunk; wts is never
// empty (one chunk of zeros).  Returns the largest k1 (0 when every filter is empty).
inline int filter_supports(const std::vector<float> &fb, int n_mels, int nb, int chunk, std::vector<int> &rows, std::vector<float> &wts) {
    rows.assign(4 * (size_t)n_mels, 0);
    wts.clear();
    int kmax = 0;
    for (int i = 0; i < n_mels; ++i) {
        int k0 = nb, k1 = 0;
        for (int k = 0; k < nb; ++k)
            if (fb[(size_t)i * nb + k] != 0.f) { k0 = k < k0 ? k : k0; k1 = k + 1; }
        if (k1 == 0) k0 = 0;
        const int nch = (k1 - k0 + chunk - 1) / chunk;
        rows[4 * i] = k0; rows[4 * i + 1] = nch; rows[4 * i + 2] = (int)wts.size();
        for (int k = k0; k < k0 + chunk * nch; ++k) wts.push_back(k < k1 ? fb[(size_t)i * nb + k] : 0.f);
        if (k1 > kmax) kmax = k1;
    }
    if (wts.empty()) wts.assign(chunk, 0.f);
    return kmax;
}

}  // namespace gtts
