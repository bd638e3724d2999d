// wav.hip -- waveform front end of the DiffVC speaker encoder (DiffVC/speaker_encoder/encoder/audio.py:50-58, 76-89, 101-114):
//   * wav_resample_kernel   torchaudio Resample with its defaults (sinc_interp_hann): y[q n + p] = sum_j k[p][j] xpad[q o + j] over the
//                           taps of phase p that the clamp leaves (17 of 459 at 22050 -> 16000; the others are 1e-49 in float64 and 0 in
//                           fp32).  The zero padding is index arithmetic.  A workgroup owns a tile of WAV_RT consecutive outputs of one
//                           row and leaves the tile's sum of y^2 beside the output.
//   * wav_normalize_kernel  normalize_volume_batch: reduces a row's tile sums in a fixed order, forms the gain, scales.  On a waveform
//                           that never went through the resampler wav_sumsq_kernel forms the same tile sums first (same tile, same
//                           order: the result is the same bit for bit).
//   * wav_powmel_kernel     the POWER mel of the encoder: reflect pad n_fft / 2, frames of n_fft at stride hop, periodic Hann window,
//                           one-sided DFT, re^2 + im^2, slaney filterbank, [B, T, n_mels] frame-major (what spk.hip reads).  The
//                           transform is dense: frames [T, n_fft] times the table [n_fft, 2 bins] (window folded in, host float64) on
//                           v_mfma_f32_16x16x4_f32 -- n_fft = 400 is 16 * 25, no power of two.  A workgroup of four waves owns WAV_TF = 16
//                           consecutive frames of one row (one MFMA column tile); wave w owns the 16-row tiles w, w + 4, ... of the
//                           table, each holding 8 bins with re and im interleaved so that both parts of a bin meet in one lane.
//                           Reflection and framing are the addressing of the loads that stage the tile's samples in LDS; the next k
//                           block's A fragments travel under the current one's MFMAs; the power goes to LDS, the n_mels short dot
//                           products (contiguous supports) read it, only the mel leaves.
// fp32 throughout; every table is computed on the host in float64 (no device sin / cos); no floating-point atomics; every sum has a
// fixed order, and an MFMA column is a frame: an output depends on its own samples and the tables, never on B, its place or the grid.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/gradtts_abi.h"
#include "common.h"
#include "kernels.h"
#include "spectral.h"

namespace gtts {

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int WAV_RT = 1024;       // outputs per resample / normalise workgroup: 256 threads, thread t owns t, t + 256, t + 512, t + 768
constexpr int WAV_TF = 16;         // frames per power-mel workgroup: the columns of one MFMA tile
constexpr int WAV_GT = 8;          // table row tiles a wave accumulates at once

// sum of v^2 over a tile in ONE order for every kernel that forms it: the thread's four squares ascending, the wave (wave_sum), the
// four waves pairwise.  Every thread returns the total.
__device__ __forceinline__ float wav_tile_sumsq(const float (&v)[4], float *red) {
#pragma clang fp contract(off)
    float s = v[0] * v[0];
    s = fmaf(v[1], v[1], s);
    s = fmaf(v[2], v[2], s);
    s = fmaf(v[3], v[3], s);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    lds_barrier();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

struct WavRsArgs {
    const float *x;                // [B][L]
    float *y;                      // [B][Lo]
    float *part;                   // [B][ntile]
    const int *first;              // [n]      first tap of the phase's support
    const float *taps;             // [S][n]   tap s of phase p at s * n + p (zeros behind a phase's support)
    int L, Lo, o, n, S, w, ntile;
};

__global__ __launch_bounds__(256) void wav_resample_kernel(WavRsArgs a) {
    __shared__ float red[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const float *x = a.x + (size_t)b * a.L;
    float *y = a.y + (size_t)b * a.Lo;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = blockIdx.x * WAV_RT + r * 256 + tid;
        v[r] = 0.f;
        if (m < a.Lo) {
            const int q = m / a.n, p = m - q * a.n;
            const long long base = (long long)q * a.o + a.first[p] - a.w;      // index into x of the phase's first tap (may lie outside)
            const float *tp = a.taps + p;
            float acc = 0.f;
            for (int s = 0; s < a.S; ++s) {
                const long long i = base + s;
                const float xv = (i >= 0 && i < a.L) ? x[i] : 0.f;
                acc = fmaf(tp[(size_t)s * a.n], xv, acc);
            }
            y[m] = acc;
            v[r] = acc;
        }
    }
    const float total = wav_tile_sumsq(v, red);
    if (tid == 0) a.part[(size_t)b * a.ntile + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void wav_sumsq_kernel(const float *x, float *part, int L, int ntile) {
    __shared__ float red[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = blockIdx.x * WAV_RT + r * 256 + tid;
        v[r] = m < L ? x[(size_t)b * L + m] : 0.f;
    }
    const float total = wav_tile_sumsq(v, red);
    if (tid == 0) part[(size_t)b * ntile + blockIdx.x] = total;
}

// mode 0: no direction (gain 1), 1: increase_only, 2: decrease_only.  A row left alone is multiplied by exactly 1, so an all-zero row
// stays 0 under modes 0 and 2, as in the drop-in's torch recipe (the reference forms 1 + 0 (inf - 1) = NaN for it in every mode).
__global__ __launch_bounds__(256) void wav_normalize_kernel(const float *x, float *y, const float *part, int L, int ntile, double target, int mode) {
    __shared__ float red[4];
    __shared__ float gain_s;
    const int tid = threadIdx.x, b = blockIdx.y;
    float s = 0.f;
    for (int i = tid; i < ntile; i += 256) s += part[(size_t)b * ntile + i];
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    lds_barrier();
    if (tid == 0) {
        const float mean = ((red[0] + red[1]) + (red[2] + red[3])) / (float)L;
        const double change = target - 10.0 * log10((double)mean);          // mean = 0: +inf, the gain inf, the row 0 * inf = NaN
        float g = 1.f;
        if ((mode == 1 && change > 0.0) || (mode == 2 && change < 0.0)) g = (float)pow(10.0, change / 20.0);
        gain_s = g;
    }
    lds_barrier();
    const float g = gain_s;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = blockIdx.x * WAV_RT + r * 256 + tid;
        if (m < L) y[(size_t)b * L + m] = x[(size_t)b * L + m] * g;
    }
}

struct WavMelArgs {
    const float *x;                // [B][L]
    float *out;                    // [B][T][n_mels]
    const float4 *dft;             // [ntl][KB][64]   A fragments of the windowed DFT table
    const int4 *rows;              // [n_mels]        {first bin, bins, offset into wts, 0}
    const float *wts;              // [nw]
    int L, T, n_fft, hop, pad, n_mels, KB, ntl, kstride, nw;
};

__global__ __launch_bounds__(256) void wav_powmel_kernel(WavMelArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wav_smem[];
    int4 *rows = reinterpret_cast<int4 *>(wav_smem);                          // [n_mels]
    float *pw = reinterpret_cast<float *>(rows + a.n_mels);                   // [WAV_TF][kstride]
    float *wts = pw + WAV_TF * a.kstride;                                     // [nw]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sq = lane & 15, q = lane >> 4;
    const int b = blockIdx.y, t0 = blockIdx.x * WAV_TF;
    const float *x = a.x + (size_t)b * a.L;
    for (int i = tid; i < a.n_mels; i += 256) rows[i] = a.rows[i];
    for (int i = tid; i < a.nw; i += 256) wts[i] = a.wts[i];
    // the tile's samples, reflected about the row's ends, once into LDS: sample j of the tile at j + j / 32, so that the 16 frames of
    // the tile, a hop apart, read different banks when the hop is a multiple of 32 (160 is)
    float *xs = wts + a.nw;                                                   // [span + span / 32 + 1]
    const int span = (WAV_TF - 1) * a.hop + a.n_fft, i0 = t0 * a.hop - a.pad;
    for (int j = tid; j < span; j += 256) {
        const int i = reflect_index(i0 + j, a.L);                             // (L > pad: one reflection is enough for a frame of the row)
        xs[j + (j >> 5)] = (i >= 0 && i < a.L) ? x[i] : 0.f;                  // (still outside: a frame behind the row's last)
    }
    lds_barrier();
    const bool live = t0 + sq < a.T;                                          // this lane's frame: column sq of the tile
    const int loc = sq * a.hop;                                               // its sample 0 in the tile's buffer
    for (int g0 = 0; g0 < a.ntl; g0 += 4 * WAV_GT) {
        f32x4 acc[WAV_GT];
        float4 wn[WAV_GT];                                                    // the next k block's A fragments, in flight under the MFMAs
#pragma unroll
        for (int i = 0; i < WAV_GT; ++i) {
            acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int tl = g0 + 4 * i + wave;
            wn[i] = tl < a.ntl ? a.dft[(size_t)tl * a.KB * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        for (int kb = 0; kb < a.KB; ++kb) {
            const int k = kb * 16 + q * 4;
            float4 wc[WAV_GT];
#pragma unroll
            for (int i = 0; i < WAV_GT; ++i) {
                const int tl = g0 + 4 * i + wave;
                wc[i] = wn[i];
                if (tl < a.ntl && kb + 1 < a.KB) wn[i] = a.dft[((size_t)tl * a.KB + kb + 1) * 64 + lane];       // (uniform over the wave)
            }
            float bv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int jj = loc + k + j;
                bv[j] = (live && k + j < a.n_fft) ? xs[jj + (jj >> 5)] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < WAV_GT; ++i) {
                if (g0 + 4 * i + wave < a.ntl) {
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[i].x, bv[0], acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[i].y, bv[1], acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[i].z, bv[2], acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[i].w, bv[3], acc[i], 0, 0, 0);
                }
            }
        }
        // rows 4 q ... 4 q + 3 of tile tl are (re, im) of bins 8 tl + 2 q and 8 tl + 2 q + 1
#pragma unroll
        for (int i = 0; i < WAV_GT; ++i) {
            const int tl = g0 + 4 * i + wave;
            if (tl < a.ntl) {
#pragma clang fp contract(off)
                float *p = pw + sq * a.kstride + 8 * tl + 2 * q;
                p[0] = fmaf(acc[i].y, acc[i].y, acc[i].x * acc[i].x);
                p[1] = fmaf(acc[i].w, acc[i].w, acc[i].z * acc[i].z);
            }
        }
    }
    lds_barrier();
    // ---- mel projection: one short dot product per (frame, band), ascending bins; lanes along the band axis, the store's contiguous one
    float *out = a.out + (size_t)b * a.T * a.n_mels;
    for (int idx = tid; idx < WAV_TF * a.n_mels; idx += 256) {
        const int f = idx / a.n_mels, i = idx - f * a.n_mels, t = t0 + f;
        if (t >= a.T) break;
        const int4 rw = rows[i];
        const float *p = pw + f * a.kstride + rw.x, *w = wts + rw.z;
        float acc = 0.f;
        for (int c = 0; c < rw.y; ++c) acc = fmaf(w[c], p[c], acc);
        out[(size_t)t * a.n_mels + i] = acc;
    }
}

}  // namespace gtts

using namespace gtts;

// host-side metadata: the configuration and the float64-computed tables, laid out as the device blob
struct gtts_wav {
    gtts_wav_cfg cfg;
    int o, n, w, S;                         // reduced rates, padding, taps kept per phase
    std::vector<int> first;                 // [n]
    std::vector<float> taps;                // [n][S] (phase-major: the host's view; the blob holds the transpose)
    int KB, ntl, kstride, nw;
    std::vector<float> fb;                  // [n_mels][n_fft/2 + 1]
    std::vector<unsigned char> image;
    size_t off_first, off_taps, off_dft, off_rows, off_wts, smem;
};

namespace {

int gcd_int(int a, int b) { return b == 0 ? a : gcd_int(b, a % b); }

hipError_t powmel_launch(const WavMelArgs &a, int B, size_t smem, hipStream_t st) {
    const hipError_t e = raise_dyn_lds<&wav_powmel_kernel>(smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wav_powmel_kernel, dim3((unsigned)((a.T + WAV_TF - 1) / WAV_TF), (unsigned)B), dim3(256), smem, st, a);
    return hipGetLastError();
}

int tiles_of(int L) { return (L + WAV_RT - 1) / WAV_RT; }

// B rows of L samples each: the element count must stay below 2^31
int check_rows(const char *what, int B, long long L) {
    if (B < 1 || B > 65535) return fail(GTTS_E_SHAPE, "%s: B must lie in [1, 65535] (got %d)", what, B);
    if (L < 1) return fail(GTTS_E_SHAPE, "%s: a row needs at least one sample (got %lld)", what, L);
    if ((long long)B * L >= (1LL << 31)) return fail(GTTS_E_SHAPE, "%s: B * L = %d * %lld reaches 2^31", what, B, L);
    return GTTS_OK;
}

}  // namespace

extern "C" int gtts_wav_create(const gtts_wav_cfg *cfg, gtts_wav **out) {
    if (!cfg || !out) return fail(GTTS_E_NULL, "gtts_wav_create: null argument");
    const gtts_wav_cfg c = *cfg;
    if (c.source_sr < 1 || c.sampling_rate < 1) return fail(GTTS_E_CONFIG, "wav: sampling rates must be positive (got %d, %d)", c.source_sr, c.sampling_rate);
    const int g = gcd_int(c.source_sr, c.sampling_rate), o = c.source_sr / g, n = c.sampling_rate / g;
    if (o > 1024 || n > 1024)
        return fail(GTTS_E_CONFIG, "wav: %d -> %d Hz reduces to %d / %d; both must be <= 1024", c.source_sr, c.sampling_rate, o, n);
    if (c.lowpass_filter_width < 1 || c.lowpass_filter_width > 64 || !(c.rolloff > 0.0) || !(c.rolloff <= 1.0))
        return fail(GTTS_E_CONFIG, "wav: need 1 <= lowpass_filter_width <= 64 and 0 < rolloff <= 1 (got %d, %g)", c.lowpass_filter_width, c.rolloff);
    if (c.n_fft < 64 || c.n_fft > 1024 || c.n_fft % 2 != 0) return fail(GTTS_E_CONFIG, "wav: n_fft must be even and lie in [64, 1024] (got %d)", c.n_fft);
    if (c.hop_size < 1 || c.hop_size > c.n_fft) return fail(GTTS_E_CONFIG, "wav: hop_size must lie in [1, n_fft] (got %d)", c.hop_size);
    if (c.n_mels < 1 || c.n_mels > 128) return fail(GTTS_E_CONFIG, "wav: n_mels must lie in [1, 128] (got %d)", c.n_mels);
    if (!(c.fmin >= 0.0) || !(c.fmax > c.fmin) || !(c.fmax <= 0.5 * c.sampling_rate))
        return fail(GTTS_E_CONFIG, "wav: need 0 <= fmin < fmax <= sampling_rate / 2 (got %g, %g, %d)", c.fmin, c.fmax, c.sampling_rate);
    gtts_wav *m = new gtts_wav();
    m->cfg = c;
    m->o = o;
    m->n = n;
    const double pi = 3.141592653589793238462643383279;
    // ---- resampling taps: k[p][j] of torchaudio's sinc_interp_hann kernel, float64, kept where the clamp does not bite
    const double lpw = c.lowpass_filter_width, base = (o < n ? o : n) * c.rolloff;
    m->w = (int)std::ceil(lpw * o / base);
    const int J = 2 * m->w + o;
    std::vector<int> last(n);
    m->first.assign(n, 0);
    m->S = 1;
    auto t_of = [&](int p, int j) { return (-(double)p / n + (double)(j - m->w) / o) * base; };
    for (int p = 0; p < n; ++p) {
        int f = -1, l = -1;
        for (int j = 0; j < J; ++j)
            if (std::fabs(t_of(p, j)) < lpw) { if (f < 0) f = j; l = j; }
        if (f < 0) f = l = 0;
        m->first[p] = f;
        last[p] = l;
        if (l - f + 1 > m->S) m->S = l - f + 1;
    }
    m->taps.assign((size_t)n * m->S, 0.f);
    for (int p = 0; p < n; ++p)
        for (int j = m->first[p]; j <= last[p]; ++j) {
            const double t = t_of(p, j), win = std::cos(t * pi / lpw / 2.0);
            const double sinc = t == 0.0 ? 1.0 : std::sin(pi * t) / (pi * t);
            m->taps[(size_t)p * m->S + (j - m->first[p])] = (float)((base / o) * win * win * sinc);
        }
    // ---- power mel: filterbank rows as contiguous supports, the windowed one-sided DFT table as MFMA A fragments
    const int N = c.n_fft, nb = N / 2 + 1;
    slaney_filterbank(c.sampling_rate, N, c.n_mels, c.fmin, c.fmax, m->fb);
    std::vector<int> rows;
    std::vector<float> wts;
    filter_supports(m->fb, c.n_mels, nb, 1, rows, wts);        // (an empty filter: the cell is 0)
    m->nw = (int)wts.size();
    m->KB = (N + 15) / 16;
    m->ntl = (nb + 7) / 8;
    m->kstride = (8 * m->ntl) | 1;        // odd: the 16 frames of a column tile write to different banks
    m->off_first = 0;
    m->off_taps = align256((size_t)n * 4);
    m->off_dft = m->off_taps + align256(m->taps.size() * 4);
    m->off_rows = m->off_dft + align256((size_t)m->ntl * m->KB * 64 * 16);
    m->off_wts = m->off_rows + align256(rows.size() * 4);
    m->image.assign(m->off_wts + align256(wts.size() * 4), 0);
    memcpy(m->image.data() + m->off_first, m->first.data(), (size_t)n * 4);
    float *taps = reinterpret_cast<float *>(m->image.data() + m->off_taps);
    for (int p = 0; p < n; ++p)
        for (int s = 0; s < m->S; ++s) taps[(size_t)s * n + p] = m->taps[(size_t)p * m->S + s];
    float *dft = reinterpret_cast<float *>(m->image.data() + m->off_dft);
    for (int tl = 0; tl < m->ntl; ++tl)
        for (int kb = 0; kb < m->KB; ++kb)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int r = lane & 15, bin = 8 * tl + r / 2, k = 16 * kb + 4 * (lane >> 4) + j;
                    double v = 0.0;
                    if (bin < nb && k < N) {
                        const double hann = hann_periodic(k, N);
                        const double ang = 2.0 * pi * (double)(((long long)bin * k) % N) / N;
                        v = (r & 1) ? -hann * std::sin(ang) : hann * std::cos(ang);
                    }
                    dft[(((size_t)tl * m->KB + kb) * 64 + lane) * 4 + j] = (float)v;
                }
    memcpy(m->image.data() + m->off_rows, rows.data(), rows.size() * 4);
    memcpy(m->image.data() + m->off_wts, wts.data(), wts.size() * 4);
    m->smem = (size_t)c.n_mels * 16 + (size_t)WAV_TF * m->kstride * 4 + (size_t)m->nw * 4;
    // ... and the tile's samples.  The largest supported configuration (n_fft = hop = 1024, 128 bands) needs 2 + 33 + 4 + 68 KB: every
    // configuration accepted above fits the 160 KB of a workgroup.
    const size_t span = (size_t)(WAV_TF - 1) * c.hop_size + N;
    m->smem += (span + span / 32 + 1) * 4;
    *out = m;
    return GTTS_OK;
}

extern "C" void gtts_wav_destroy(gtts_wav *m) { delete m; }

extern "C" int gtts_wav_resampled_length(const gtts_wav *m, int L) {
    if (!m) return fail(GTTS_E_NULL, "gtts_wav_resampled_length: null handle");
    if (L < 1) return fail(GTTS_E_SHAPE, "wav: a row needs at least one sample (got %d)", L);
    const long long Lo = ((long long)m->n * L + m->o - 1) / m->o;
    if (Lo >= (1LL << 31)) return fail(GTTS_E_SHAPE, "wav: %d samples resample to %lld, which reaches 2^31", L, Lo);
    return (int)Lo;
}

extern "C" int gtts_wav_frames(const gtts_wav *m, int L) {
    if (!m) return fail(GTTS_E_NULL, "gtts_wav_frames: null handle");
    if (L < 1) return fail(GTTS_E_SHAPE, "wav: a row needs at least one sample (got %d)", L);
    if (L <= m->cfg.n_fft / 2) return fail(GTTS_E_SHAPE, "wav: %d samples cannot be reflect-padded by %d (needs L > n_fft / 2)", L, m->cfg.n_fft / 2);
    if (L > 0x7fffffff - m->cfg.n_fft) return fail(GTTS_E_SHAPE, "wav: %d samples are too many for 32-bit sample indices", L);
    return 1 + L / m->cfg.hop_size;
}

extern "C" int gtts_wav_tiles(const gtts_wav *m, int L) {
    if (!m) return fail(GTTS_E_NULL, "gtts_wav_tiles: null handle");
    if (L < 1 || L > 0x7fffffff - WAV_RT) return fail(GTTS_E_SHAPE, "wav: rows of %d samples have no tile count", L);
    return tiles_of(L);
}

extern "C" int gtts_wav_span(const gtts_wav *m) { return m ? m->S : fail(GTTS_E_NULL, "gtts_wav_span: null handle"); }

extern "C" int gtts_wav_taps(const gtts_wav *m, int *first_host, float *taps_host) {
    if (!m || !first_host || !taps_host) return fail(GTTS_E_NULL, "gtts_wav_taps: null argument");
    memcpy(first_host, m->first.data(), m->first.size() * 4);
    memcpy(taps_host, m->taps.data(), m->taps.size() * 4);
    return GTTS_OK;
}

extern "C" int gtts_wav_filterbank(const gtts_wav *m, float *host_out) {
    if (!m || !host_out) return fail(GTTS_E_NULL, "gtts_wav_filterbank: null argument");
    memcpy(host_out, m->fb.data(), m->fb.size() * 4);
    return GTTS_OK;
}

extern "C" size_t gtts_wav_packed_bytes(const gtts_wav *m) { return m ? m->image.size() : 0; }

extern "C" int gtts_wav_pack(const gtts_wav *m, void *packed, gtts_stream_t stream) {
    if (!m || !packed) return fail(GTTS_E_NULL, "gtts_wav_pack: null argument");
    GTTS_HIPCHK(hipMemcpyAsync(packed, m->image.data(), m->image.size(), hipMemcpyHostToDevice, (hipStream_t)stream));
    return GTTS_OK;
}

extern "C" size_t gtts_wav_workspace_bytes(const gtts_wav *m, int B, int L) {
    if (!m || B < 1 || L < 1 || L > 0x7fffffff - WAV_RT) return 0;
    return align256((size_t)B * tiles_of(L) * 4);
}

extern "C" int gtts_wav_resample(const gtts_wav *m, const void *packed, const float *wav, float *out, float *partials, int B, int L,
                                 gtts_stream_t stream) {
    if (!m || !packed || !wav || !out || !partials) return fail(GTTS_E_NULL, "gtts_wav_resample: null argument");
    if (m->o == m->n) return fail(GTTS_E_CONFIG, "gtts_wav_resample: source and target rate are both %d Hz; there is nothing to resample", m->cfg.sampling_rate);
    int rc = check_rows("gtts_wav_resample", B, L);
    if (rc != GTTS_OK) return rc;
    const int Lo = gtts_wav_resampled_length(m, L);
    if (Lo < 0) return Lo;
    if ((rc = check_rows("gtts_wav_resample (output)", B, Lo)) != GTTS_OK) return rc;
    const unsigned char *blob = static_cast<const unsigned char *>(packed);
    WavRsArgs a;
    a.x = wav; a.y = out; a.part = partials;
    a.first = reinterpret_cast<const int *>(blob + m->off_first);
    a.taps = reinterpret_cast<const float *>(blob + m->off_taps);
    a.L = L; a.Lo = Lo; a.o = m->o; a.n = m->n; a.S = m->S; a.w = m->w; a.ntile = tiles_of(Lo);
    hipLaunchKernelGGL(wav_resample_kernel, dim3((unsigned)a.ntile, (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}

extern "C" int gtts_wav_normalize(const gtts_wav *m, const float *wav, const float *partials, double target_dBFS, int mode, float *out,
                                  void *workspace, size_t workspace_bytes, int B, int L, gtts_stream_t stream) {
    if (!m || !wav || !out) return fail(GTTS_E_NULL, "gtts_wav_normalize: null argument");
    if (mode < 0 || mode > 2) return fail(GTTS_E_CONFIG, "gtts_wav_normalize: mode must be 0 (none), 1 (increase only) or 2 (decrease only), got %d", mode);
    const int rc = check_rows("gtts_wav_normalize", B, L);
    if (rc != GTTS_OK) return rc;
    const int ntile = tiles_of(L);
    hipStream_t st = (hipStream_t)stream;
    if (!partials) {
        if (!workspace) return fail(GTTS_E_NULL, "gtts_wav_normalize: without partials a workspace is needed");
        if (workspace_bytes < gtts_wav_workspace_bytes(m, B, L))
            return fail(GTTS_E_WORKSPACE, "gtts_wav_normalize: workspace of %zu bytes, %zu needed", workspace_bytes, gtts_wav_workspace_bytes(m, B, L));
        hipLaunchKernelGGL(wav_sumsq_kernel, dim3((unsigned)ntile, (unsigned)B), dim3(256), 0, st, wav, static_cast<float *>(workspace), L, ntile);
        GTTS_HIPCHK(hipGetLastError());
        partials = static_cast<const float *>(workspace);
    }
    hipLaunchKernelGGL(wav_normalize_kernel, dim3((unsigned)ntile, (unsigned)B), dim3(256), 0, st, wav, out, partials, L, ntile, target_dBFS, mode);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}

extern "C" int gtts_wav_powmel(const gtts_wav *m, const void *packed, const float *wav, float *out, int B, int L, gtts_stream_t stream) {
    if (!m || !packed || !wav || !out) return fail(GTTS_E_NULL, "gtts_wav_powmel: null argument");
    const int rc = check_rows("gtts_wav_powmel", B, L);
    if (rc != GTTS_OK) return rc;
    const int T = gtts_wav_frames(m, L);
    if (T < 0) return T;
    if ((long long)B * T * m->cfg.n_mels >= (1LL << 31))
        return fail(GTTS_E_SHAPE, "gtts_wav_powmel: B * T * n_mels = %d * %d * %d reaches 2^31", B, T, m->cfg.n_mels);
    const unsigned char *blob = static_cast<const unsigned char *>(packed);
    WavMelArgs a;
    a.x = wav; a.out = out;
    a.dft = reinterpret_cast<const float4 *>(blob + m->off_dft);
    a.rows = reinterpret_cast<const int4 *>(blob + m->off_rows);
    a.wts = reinterpret_cast<const float *>(blob + m->off_wts);
    a.L = L; a.T = T; a.n_fft = m->cfg.n_fft; a.hop = m->cfg.hop_size; a.pad = m->cfg.n_fft / 2; a.n_mels = m->cfg.n_mels;
    a.KB = m->KB; a.ntl = m->ntl; a.kstride = m->kstride; a.nw = m->nw;
    GTTS_HIPCHK(powmel_launch(a, B, m->smem, (hipStream_t)stream));
    return GTTS_OK;
}
