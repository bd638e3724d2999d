// fgl.hip -- Fast Griffin-Lim, log-mel [B,n_mels,T] -> waveform [B,L], L = hop (T - 1): the FastGL module of DiffVC/model/utils.py:42-110.
//   c = P exp(logmel) (P: the caller's pseudo-inverse of the mel filterbank, [K][n_mels], K = n_fft / 2 + 1), x0 = istft(c + 0i), then
//   n_iters times  s = stft(x),  a = s / sqrt(max(re^2 + im^2, 1e-8)),  x = istft(c (a + m (a - a_prev))),  a_prev = a  (a_prev = 0 first);
//   stft / istft with center = True (reflect pad n_fft / 2), the periodic Hann window of n_fft samples, hop_size.
// Launches: one projection, one first inverse transform, ONE per iteration, one that materialises x.  Layout of an iteration, as in
// mel.hip (the transform itself: spectral.h): a workgroup of four waves owns a tile of FGL_TF = 16 consecutive frames of one row, a frame is transformed by one wave
// alone, in two bank-swizzled LDS buffers of that wave:
//   * sample load: either from x [B][L] (gtts_fgl_step) or gathered from the previous launch's windowed inverse frames
//     y [B][T][n_fft] as  x[j] = (sum_t y[t][p - t hop]) / (sum_t w^2[p - t hop]),  p = j + n_fft / 2,  t ascending (fgl_ola: the one
//     definition the materialising kernel uses too, so x never has to exist between iterations); reflection is index arithmetic;
//   * forward: n_fft real samples packed as n_fft / 2 complex points, Stockham autosort FFT (spectral.h), the real spectrum of
//     bins k and n_fft / 2 - k together from Z[k] and Z[M - k]; ALL K bins are formed;
//   * phase, momentum and magnitude on those two bins in registers; a is stored, s' never is;
//   * inverse: the two bins are packed back into Z'[k], Z'[M - k], conjugated, the same FFT runs again (ifft(Z) = conj(fft(conj Z))),
//     the result times w / n_fft goes to this launch's y buffer.  The imaginary parts of DC and Nyquist are dropped (c2r).
// Two y buffers alternate: a launch reads one and writes the other, so iterations are ordered by stream order alone -- no workgroup
// ever waits for another, and no value is accumulated with atomics.  A row's result depends on that row's mel and the tables alone.
// Tables (window, w^2, twiddles) are computed on the host in float64 and rounded to fp32; there is no device sin / cos.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/gradtts_abi.h"
#include "common.h"
#include "kernels.h"
#include "spectral.h"

namespace gtts {

constexpr int FGL_TF = 16;         // frames per workgroup
constexpr int FGL_WAVES = 4;       // waves per workgroup
constexpr int FGL_PT = 64;         // frames per workgroup of the projection

struct FglArgs {
    const float *x;                // [B][L] sample source, or nullptr: gather from yin
    const float *yin;              // [B][T][n_fft] windowed inverse frames of the previous launch
    float *yout;                   // [B][T][n_fft]
    const float *c;                // magnitudes, element (b, k, t) at b c_sb + k c_sk + t c_st
    const float2 *a_prev;          // phases of the previous iteration (nullptr: zero), same addressing as a_out
    float2 *a_out;                 // element (b, k, t) at b a_sb + k a_sk + t a_st
    const float *win, *win2;       // [n_fft] w, w^2
    const float2 *twm;             // [n_fft/2]       e^{-2 pi i k / (n_fft/2)}
    const float2 *twn;             // [n_fft/4 + 1]   e^{-2 pi i k / n_fft}
    size_t c_sb, a_sb;
    int c_sk, c_st, a_sk, a_st;
    int T, L, hop, init;           // init: s' = c + 0i, no forward transform (the first inverse transform)
    float mom;
};

// Sample j of the overlap-added, envelope-normalised, trimmed signal of a row's windowed inverse frames y [T][n]: position p = j + n / 2
// of the untrimmed signal is covered by the frames t with t hop <= p < t hop + n (at most ceil(n / hop)); they are summed in
// ascending t.  The ONE definition of x: the iteration's sample load and the materialising kernel return the same bits.
__device__ __forceinline__ float fgl_ola(const float *y, const float *win2, int j, int n, int T, int hop) {
    const int p = j + n / 2;
    const int tlo = p >= n ? (p - n) / hop + 1 : 0, thi = min(T - 1, p / hop);
    float s = 0.f, e = 0.f;
    for (int t = tlo; t <= thi; ++t) {
        const int o = p - t * hop;
        s += y[(size_t)t * n + o];
        e += win2[o];
    }
    return s / e;
}

// The wave's FFT (spectral.h) with the M-point twiddle table `tw` read from LDS.  (Held in registers per lane, as mel.hip does, the
// pass twiddles cost 48 VGPRs at n_fft = 1024 and 120 at 2048 and, with the window, kept the kernel at one wave per SIMD; read from
// LDS it runs at three, at 2048 at two.)
template <int LOGN>
__device__ __forceinline__ void fgl_fft(float2 *&x, float2 *&y, const float2 *tw, int lane) {
    stockham_fft<LOGN>(x, y, [tw](int, int, int ps, int m) { return tw[m * ps]; }, lane);
}

// s / sqrt(max(re^2 + im^2, 1e-8))
__device__ __forceinline__ float2 fgl_phase(float2 s) {
    const float d = sqrtf(fmaxf(s.x * s.x + s.y * s.y, 1e-8f));
    return make_float2(s.x / d, s.y / d);
}

// c (a + m (a - a_prev)), in the reference's order of operations
__device__ __forceinline__ float2 fgl_update(float c, float2 a, float2 prev, float m) {
    return make_float2(c * (a.x + m * (a.x - prev.x)), c * (a.y + m * (a.y - prev.y)));
}

template <int LOGN>
__global__ __launch_bounds__(64 * FGL_WAVES) void fgl_kernel(FglArgs a) {
    constexpr int N = 1 << LOGN, M = N / 2, R = M / 64, H = M / 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char fgl_smem[];
    float2 *tw = reinterpret_cast<float2 *>(fgl_smem);                       // [M]
    float2 *twn = tw + M;                                                    // [H + 2]
    float2 *bufs = twn + H + 2;                                              // [FGL_WAVES][2][M]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * FGL_TF;
    for (int i = tid; i < M; i += 64 * FGL_WAVES) tw[i] = a.twm[i];
    for (int i = tid; i <= H; i += 64 * FGL_WAVES) twn[i] = a.twn[i];
    const float2 *win = reinterpret_cast<const float2 *>(a.win);         // read at both uses: 4 to 16 KB, cache resident
    lds_barrier();

    const float *xrow = a.x ? a.x + (size_t)b * a.L : nullptr;
    const float *yrow = a.yin ? a.yin + (size_t)b * a.T * N : nullptr;
    const float *crow = a.c + (size_t)b * a.c_sb;
    const float2 *prow = a.a_prev ? a.a_prev + (size_t)b * a.a_sb : nullptr;
    float2 *arow = a.a_out ? a.a_out + (size_t)b * a.a_sb : nullptr;
    constexpr float scale = 1.0f / (float)N;
#pragma unroll 1
    for (int f = wave; f < FGL_TF; f += FGL_WAVES) {
        const int t = t0 + f;
        if (t >= a.T) break;
        float2 *x = bufs + wave * 2 * M, *y = x + M;
        if (!a.init) {
            // frame t of stft(x, center = True): samples t hop - N / 2 + n, reflected about the row's ends (L > N / 2)
            const int base = t * a.hop - N / 2;
#pragma unroll 1
            for (int r = 0; r < R; ++r) {
                const int j = base + 2 * (lane + 64 * r), j0 = reflect_index(j, a.L), j1 = reflect_index(j + 1, a.L);
                float v0, v1;
                if (xrow) { v0 = xrow[j0]; v1 = xrow[j1]; }
                else { v0 = fgl_ola(yrow, a.win2, j0, N, a.T, a.hop); v1 = fgl_ola(yrow, a.win2, j1, N, a.T, a.hop); }
                const float2 w = win[lane + 64 * r];
                x[fft_at(lane + 64 * r)] = make_float2(v0 * w.x, v1 * w.y);
            }
            wave_lds_sync();
            fgl_fft<LOGN>(x, y, tw, lane);
        }
        // ---- bins k and M - k (k = 0: DC and Nyquist) from Z[k], Z[M - k]; phase, momentum, magnitude; packed back into y
#pragma unroll 1
        for (int k = lane; k <= H; k += 64) {
            const int k2 = M - k;
            const float2 w = twn[k];
            float2 sk = make_float2(crow[(size_t)k * a.c_sk + (size_t)t * a.c_st], 0.f);
            float2 sm = make_float2(crow[(size_t)k2 * a.c_sk + (size_t)t * a.c_st], 0.f);
            if (!a.init) {
                const RealSplit sp = real_split(x[fft_at(k & (M - 1))], x[fft_at(k2 & (M - 1))], w);
                const float2 ak = fgl_phase(make_float2(sp.e.x + sp.wo.x, sp.e.y + sp.wo.y));         // X[k] = E + W^k O
                const float2 am = fgl_phase(make_float2(sp.e.x - sp.wo.x, -(sp.e.y - sp.wo.y)));      // X[M-k] = conj(E - W^k O)
                const size_t ik = (size_t)k * a.a_sk + (size_t)t * a.a_st, im = (size_t)k2 * a.a_sk + (size_t)t * a.a_st;
                float2 pk = make_float2(0.f, 0.f), pm = pk;
                if (prow) { pk = prow[ik]; pm = prow[im]; }
                sk = fgl_update(sk.x, ak, pk, a.mom);
                sm = fgl_update(sm.x, am, pm, a.mom);
                arow[ik] = ak;
                if (k2 != k) arow[im] = am;
            }
            if (k == 0) { sk.y = 0.f; sm.y = 0.f; }                                           // c2r ignores them
            // Z'[k] = E' + i O', Z'[M-k] = conj E' + i conj O' with E' = S[k] + conj S[M-k], O' = (S[k] - conj S[M-k]) conj W^k
            // (the factor 1 / 2 of both is in `scale`)
            const float epr = sk.x + sm.x, epi = sk.y - sm.y, dr = sk.x - sm.x, di = sk.y + sm.y;
            const float opr = dr * w.x + di * w.y, opi = di * w.x - dr * w.y;
            y[fft_at(k & (M - 1))] = make_float2(epr - opi, -(epi + opr));                    // conj Z'[k]
            if (k != 0 && k2 != k) y[fft_at(k2)] = make_float2(epr + opi, -(opr - epi));      // conj Z'[M-k]
        }
        wave_lds_sync();
        { float2 *tmp = x; x = y; y = tmp; }
        fgl_fft<LOGN>(x, y, tw, lane);
        // z[m] = conj(fft(conj Z'))[m] / N = x[2m] + i x[2m+1]; windowed, stored as frame t of y
        float2 *yo = reinterpret_cast<float2 *>(a.yout + ((size_t)b * a.T + t) * N);
#pragma unroll 1
        for (int r = 0; r < R; ++r) {
            const float2 z = x[fft_at(lane + 64 * r)], w = win[lane + 64 * r];
            yo[lane + 64 * r] = make_float2((z.x * scale) * w.x, (-z.y * scale) * w.y);
        }
        wave_lds_sync();                  // the next frame overwrites this wave's buffers
    }
}

// c[b, k, t] = sum_m P[k, m] exp(logmel[b, m, t]): a workgroup owns FGL_PT frames of one row, lanes along the frame axis, a wave walks
// the bins k = wave, wave + 4, ... ; the sum runs over m in four interleaved chains combined as (0 + 1) + (2 + 3).
__global__ __launch_bounds__(256) void fgl_project_kernel(const float *logmel, const float *P, float *c, int n_mels, int K, int T, size_t c_sb,
                                                          int c_sk, int c_st) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fgl_smem[];
    float *E = reinterpret_cast<float *>(fgl_smem);                          // [n_mels][FGL_PT]
    const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * FGL_PT;
    const float *row = logmel + (size_t)b * n_mels * T;
    for (int idx = tid; idx < n_mels * FGL_PT; idx += 256) {
        const int m = idx / FGL_PT, t = t0 + (idx & (FGL_PT - 1));
        E[idx] = t < T ? expf(row[(size_t)m * T + t]) : 0.f;
    }
    __syncthreads();
    const int tt = tid & (FGL_PT - 1), t = t0 + tt, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (t >= T) return;
    float *out = c + (size_t)b * c_sb + (size_t)t * c_st;
    for (int k = wave; k < K; k += 4) {
        const float *p = P + (size_t)k * n_mels;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int m = 0;
        for (; m + 3 < n_mels; m += 4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = fmaf(p[m + i], E[(m + i) * FGL_PT + tt], acc[i]);
        }
        for (int i = 0; m < n_mels; ++m, ++i) acc[i] = fmaf(p[m], E[m * FGL_PT + tt], acc[i]);
        out[(size_t)k * c_sk] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    }
}

// x [B][L] from the windowed inverse frames
__global__ __launch_bounds__(256) void fgl_materialise_kernel(const float *y, const float *win2, float *x, int n, int T, int L, int hop) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j < L) x[(size_t)b * L + j] = fgl_ola(y + (size_t)b * T * n, win2, j, n, T, hop);
}

}  // namespace gtts

using namespace gtts;

// host-side metadata: the configuration and the float64-computed tables, laid out as the head of the device blob
struct gtts_fgl {
    gtts_fgl_cfg cfg;
    int logn, K;
    std::vector<unsigned char> image;       // window, w^2, twiddles (the pseudo-inverse follows in the blob)
    size_t off_win, off_win2, off_twm, off_twn, off_p, bytes, smem;
};

namespace {

struct FglWs { size_t c, a, y0, y1, total; };

FglWs fgl_ws(const gtts_fgl *g, int B, int T) {
    FglWs w;
    const size_t cells = (size_t)B * T * g->K, frames = (size_t)B * T * g->cfg.n_fft;
    w.c = 0;
    w.a = w.c + align256(cells * 4);
    w.y0 = w.a + align256(cells * 8);
    w.y1 = w.y0 + align256(frames * 4);
    w.total = w.y1 + align256(frames * 4);
    return w;
}

template <int LOGN>
hipError_t fgl_launch(const FglArgs &a, int B, size_t smem, hipStream_t st) {
    const hipError_t e = raise_dyn_lds<&fgl_kernel<LOGN>>(smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fgl_kernel<LOGN>, dim3((unsigned)((a.T + FGL_TF - 1) / FGL_TF), (unsigned)B), dim3(64 * FGL_WAVES), smem, st, a);
    return hipGetLastError();
}

hipError_t fgl_transform(const gtts_fgl *g, const FglArgs &a, int B, hipStream_t st) {
    switch (g->logn) {
        case 8: return fgl_launch<8>(a, B, g->smem, st);
        case 9: return fgl_launch<9>(a, B, g->smem, st);
        case 10: return fgl_launch<10>(a, B, g->smem, st);
        default: return fgl_launch<11>(a, B, g->smem, st);
    }
}

FglArgs fgl_args(const gtts_fgl *g, const void *packed, int T) {
    const unsigned char *blob = static_cast<const unsigned char *>(packed);
    FglArgs a;
    memset(&a, 0, sizeof a);
    a.win = reinterpret_cast<const float *>(blob + g->off_win);
    a.win2 = reinterpret_cast<const float *>(blob + g->off_win2);
    a.twm = reinterpret_cast<const float2 *>(blob + g->off_twm);
    a.twn = reinterpret_cast<const float2 *>(blob + g->off_twn);
    a.T = T; a.L = g->cfg.hop_size * (T - 1); a.hop = g->cfg.hop_size; a.mom = (float)g->cfg.momentum;
    return a;
}

hipError_t fgl_project(const gtts_fgl *g, const void *packed, const float *logmel, float *c, size_t c_sb, int c_sk, int c_st, int B, int T,
                       hipStream_t st) {
    const float *P = reinterpret_cast<const float *>(static_cast<const unsigned char *>(packed) + g->off_p);
    hipLaunchKernelGGL(fgl_project_kernel, dim3((unsigned)((T + FGL_PT - 1) / FGL_PT), (unsigned)B), dim3(256),
                       (size_t)g->cfg.n_mels * FGL_PT * 4, st, logmel, P, c, g->cfg.n_mels, g->K, T, c_sb, c_sk, c_st);
    return hipGetLastError();
}

hipError_t fgl_materialise(const gtts_fgl *g, const FglArgs &a, const float *y, float *x, int B, hipStream_t st) {
    hipLaunchKernelGGL(fgl_materialise_kernel, dim3((unsigned)((a.L + 255) / 256), (unsigned)B), dim3(256), 0, st, y, a.win2, x,
                       g->cfg.n_fft, a.T, a.L, a.hop);
    return hipGetLastError();
}

// the shape checks every entry point shares; returns L or an error
int fgl_shape(const gtts_fgl *g, int B, int T, const char *who) {
    if (B <= 0 || B > 65535) return fail(GTTS_E_SHAPE, "%s: B must lie in [1, 65535] (got %d)", who, B);
    return gtts_fgl_samples(g, T);
}

}  // namespace

extern "C" int gtts_fgl_create(const gtts_fgl_cfg *cfg, gtts_fgl **out) {
    if (!cfg || !out) return fail(GTTS_E_NULL, "gtts_fgl_create: null argument");
    const gtts_fgl_cfg c = *cfg;
    int logn = 0;
    while ((1 << logn) < c.n_fft) ++logn;
    if (c.n_fft < 256 || c.n_fft > 2048 || (1 << logn) != c.n_fft)
        return fail(GTTS_E_CONFIG, "fgl: n_fft must be a power of two from 256 to 2048 (got %d)", c.n_fft);
    if (c.hop_size < 1 || c.hop_size > c.n_fft / 2)
        return fail(GTTS_E_CONFIG, "fgl: hop_size must lie in [1, n_fft / 2] (got %d)", c.hop_size);
    if (c.n_mels < 1 || c.n_mels > 128) return fail(GTTS_E_CONFIG, "fgl: n_mels must lie in [1, 128] (got %d)", c.n_mels);
    if (!(c.momentum >= 0.0) || !(c.momentum < 1.0)) return fail(GTTS_E_CONFIG, "fgl: momentum must lie in [0, 1) (got %g)", c.momentum);
    gtts_fgl *g = new gtts_fgl();
    g->cfg = c;
    g->logn = logn;
    const int N = c.n_fft, M = N / 2, H = M / 2;
    g->K = M + 1;
    g->off_win = 0;
    g->off_win2 = g->off_win + align256((size_t)N * 4);
    g->off_twm = g->off_win2 + align256((size_t)N * 4);
    g->off_twn = g->off_twm + align256((size_t)M * 8);
    g->off_p = g->off_twn + align256((size_t)(H + 1) * 8);
    g->bytes = g->off_p + align256((size_t)g->K * c.n_mels * 4);
    g->image.assign(g->off_p, 0);
    float *win = reinterpret_cast<float *>(g->image.data() + g->off_win), *win2 = reinterpret_cast<float *>(g->image.data() + g->off_win2);
    float *twm = reinterpret_cast<float *>(g->image.data() + g->off_twm), *twn = reinterpret_cast<float *>(g->image.data() + g->off_twn);
    for (int n = 0; n < N; ++n) {
        const double w = hann_periodic(n, N);
        win[n] = (float)w;
        win2[n] = (float)(w * w);
    }
    fill_twiddles(twm, M, M);
    fill_twiddles(twn, H + 1, N);
    g->smem = (size_t)M * 8 + (size_t)(H + 2) * 8 + (size_t)FGL_WAVES * 2 * M * 8;
    *out = g;
    return GTTS_OK;
}

extern "C" void gtts_fgl_destroy(gtts_fgl *g) { delete g; }

extern "C" int gtts_fgl_samples(const gtts_fgl *g, int T) {
    if (!g) return fail(GTTS_E_NULL, "gtts_fgl_samples: null handle");
    const int N = g->cfg.n_fft, hop = g->cfg.hop_size;
    if (T < 1 || (long long)hop * (T - 1) <= N / 2)
        return fail(GTTS_E_SHAPE, "fgl: %d frames give %lld samples, which cannot be reflect-padded by %d (needs at least %d frames)", T,
                    (long long)hop * (T > 0 ? T - 1 : 0), N / 2, (N / 2) / hop + 2);
    if ((long long)hop * (T - 1) + 2LL * N > 0x7fffffffLL || (long long)T * g->K > 0x7fffffffLL)
        return fail(GTTS_E_SHAPE, "fgl: %d frames are too many for 32-bit sample indices", T);
    return hop * (T - 1);
}

extern "C" size_t gtts_fgl_packed_bytes(const gtts_fgl *g) { return g ? g->bytes : 0; }

extern "C" int gtts_fgl_pack(const gtts_fgl *g, const float *inv_basis_host, void *packed, gtts_stream_t stream) {
    if (!g || !inv_basis_host || !packed) return fail(GTTS_E_NULL, "gtts_fgl_pack: null argument");
    hipStream_t st = (hipStream_t)stream;
    GTTS_HIPCHK(hipMemcpyAsync(packed, g->image.data(), g->image.size(), hipMemcpyHostToDevice, st));
    GTTS_HIPCHK(hipMemcpyAsync(static_cast<unsigned char *>(packed) + g->off_p, inv_basis_host, (size_t)g->K * g->cfg.n_mels * 4,
                               hipMemcpyHostToDevice, st));
    GTTS_HIPCHK(hipStreamSynchronize(st));        // the caller's matrix may be a temporary
    return GTTS_OK;
}

extern "C" size_t gtts_fgl_workspace_bytes(const gtts_fgl *g, int B, int T) {
    if (!g || B <= 0 || T <= 0) return 0;
    return fgl_ws(g, B, T).total;
}

extern "C" int gtts_fgl_init(const gtts_fgl *g, const void *packed, const float *logmel, float *c, float *x0, void *workspace,
                             size_t workspace_bytes, int B, int T, gtts_stream_t stream) {
    if (!g || !packed || !logmel || !c || !x0 || !workspace) return fail(GTTS_E_NULL, "gtts_fgl_init: null argument");
    const int L = fgl_shape(g, B, T, "gtts_fgl_init");
    if (L < 0) return L;
    const FglWs w = fgl_ws(g, B, T);
    if (workspace_bytes < w.total) return fail(GTTS_E_WORKSPACE, "gtts_fgl_init: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float *y0 = reinterpret_cast<float *>(static_cast<unsigned char *>(workspace) + w.y0);
    GTTS_HIPCHK(fgl_project(g, packed, logmel, c, (size_t)g->K * T, T, 1, B, T, st));
    FglArgs a = fgl_args(g, packed, T);
    a.init = 1; a.yout = y0; a.c = c; a.c_sb = (size_t)g->K * T; a.c_sk = T; a.c_st = 1;
    GTTS_HIPCHK(fgl_transform(g, a, B, st));
    GTTS_HIPCHK(fgl_materialise(g, a, y0, x0, B, st));
    return GTTS_OK;
}

extern "C" int gtts_fgl_step(const gtts_fgl *g, const void *packed, const float *c, const float *x_in, const float *a_prev, float *x_out,
                             float *a_out, void *workspace, size_t workspace_bytes, int B, int T, gtts_stream_t stream) {
    if (!g || !packed || !c || !x_in || !a_prev || !x_out || !a_out || !workspace) return fail(GTTS_E_NULL, "gtts_fgl_step: null argument");
    const int L = fgl_shape(g, B, T, "gtts_fgl_step");
    if (L < 0) return L;
    const FglWs w = fgl_ws(g, B, T);
    if (workspace_bytes < w.total) return fail(GTTS_E_WORKSPACE, "gtts_fgl_step: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float *y0 = reinterpret_cast<float *>(static_cast<unsigned char *>(workspace) + w.y0);
    FglArgs a = fgl_args(g, packed, T);
    a.x = x_in; a.yout = y0;
    a.c = c; a.c_sb = (size_t)g->K * T; a.c_sk = T; a.c_st = 1;
    a.a_prev = reinterpret_cast<const float2 *>(a_prev); a.a_out = reinterpret_cast<float2 *>(a_out);
    a.a_sb = (size_t)g->K * T; a.a_sk = T; a.a_st = 1;
    GTTS_HIPCHK(fgl_transform(g, a, B, st));
    GTTS_HIPCHK(fgl_materialise(g, a, y0, x_out, B, st));
    return GTTS_OK;
}

extern "C" int gtts_fgl_forward(const gtts_fgl *g, const void *packed, const float *logmel, float *wav, void *workspace, size_t workspace_bytes,
                                int B, int T, int n_iters, gtts_stream_t stream) {
    if (!g || !packed || !logmel || !wav || !workspace) return fail(GTTS_E_NULL, "gtts_fgl_forward: null argument");
    if (n_iters < 0) return fail(GTTS_E_SHAPE, "gtts_fgl_forward: n_iters must not be negative (got %d)", n_iters);
    const int L = fgl_shape(g, B, T, "gtts_fgl_forward");
    if (L < 0) return L;
    const FglWs w = fgl_ws(g, B, T);
    if (workspace_bytes < w.total) return fail(GTTS_E_WORKSPACE, "gtts_fgl_forward: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *c = reinterpret_cast<float *>(ws + w.c);
    float2 *ph = reinterpret_cast<float2 *>(ws + w.a);
    float *y[2] = {reinterpret_cast<float *>(ws + w.y0), reinterpret_cast<float *>(ws + w.y1)};
    // inside the call c and the phases are frame-major [B][T][K]: the lanes of a frame's wave run along k
    GTTS_HIPCHK(fgl_project(g, packed, logmel, c, (size_t)g->K * T, 1, g->K, B, T, st));
    FglArgs a = fgl_args(g, packed, T);
    a.c = c; a.c_sb = (size_t)g->K * T; a.c_sk = 1; a.c_st = g->K;
    a.a_sb = (size_t)g->K * T; a.a_sk = 1; a.a_st = g->K;
    a.init = 1; a.yout = y[0];
    GTTS_HIPCHK(fgl_transform(g, a, B, st));
    a.init = 0; a.a_out = ph;
    for (int it = 0; it < n_iters; ++it) {
        a.yin = y[it & 1]; a.yout = y[(it + 1) & 1];
        a.a_prev = it == 0 ? nullptr : ph;        // a cell's phase is read and rewritten by the one lane that owns it
        GTTS_HIPCHK(fgl_transform(g, a, B, st));
    }
    GTTS_HIPCHK(fgl_materialise(g, a, y[n_iters & 1], wav, B, st));
    return GTTS_OK;
}
