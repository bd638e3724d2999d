// mel_train.hip -- input gradient of the log-mel front end (mel.hip): dmel [B,num_mels,T] -> dwav [B,L] for
//   mel = log(max(W sqrt(re^2 + im^2 + 1e-9), 1e-5)),  rows reflect-padded about their own ends, frames of n_fft at stride hop.
// Nothing but the waveform is kept from the forward; per frame t < Tb of row b everything is formed again:
//   frame -> window -> FFT -> X[k], mag[k], acc[i] = sum_k W[i,k] mag[k]       (the forward's device code and summation order: mel.h)
//   dacc[i] = dmel[i,t] / acc[i] where acc[i] >= 1e-5, else 0                  (torch's clamp(min=) gradient: it passes at equality)
//   dmag[k] = sum_i W[i,k] dacc[i]                                             (the transposed table: a contiguous row range per bin)
//   G[k]    = dmag[k] X[k] / mag[k] for k < kmax, 0 above                      (mag >= sqrt(1e-9): no division by zero)
//   g[n]    = Re sum_{k=0}^{N/2} G[k] e^{+2 pi i k n / N}                      (the ADJOINT of the one-sided DFT, not irfft: in Hermitian
//             form H[0] = Re G[0], H[N/2] = Re G[N/2], H[k] = G[k] / 2, H[N-k] = conj(G[k]) / 2, unnormalised)
//   dframe[n] = g[n] win[n].
// Two launches, as fgl.hip does it, and no floating-point atomics:
//   1. mel_bwd_frames_kernel: ONE wave owns one frame from its sample load to the store of dframe into the caller's workspace
//      [B][T][n_fft]; no workgroup barrier inside a frame.  The inverse runs as an M = n_fft / 2 point transform through the inverse
//      of real_split (fgl.hip's packing of Z'[k], Z'[M-k]) and the forward FFT on conjugates.  A workgroup of four waves shares the
//      tables in LDS and owns `tf` consecutive frames of a row; tf is a launch argument (4 or 8) chosen so that small launches
//      still fill the chip -- a frame's bits do not depend on it.
//   2. mel_bwd_gather_kernel: the adjoint of framing and reflect padding.  Sample j < len collects from the padded positions q = j,
//      q = -j (1 <= j <= pad) and q = 2 (len - 1) - j (where that lies in the right pad), in this order, and for each from every
//      frame t < Tb with 0 <= q + pad - t hop < n_fft in ascending t.  Samples at or beyond len get 0.
// A row's gradient depends on that row's samples, its dmel and the tables alone: not on B, the tile size or the grid.
#include <hip/hip_runtime.h>

#include "../../include/gradtts_abi.h"
#include "common.h"
#include "kernels.h"
#include "mel.h"
#include "spectral.h"

namespace gtts {

struct MelBwdArgs {
    MelArgs f;                     // the forward's arguments (out is unused)
    const float *dmel;             // [B][num_mels][T]
    const int4 *cols;              // [kmax]            {first row, rows, offset into wtt, 0}
    const float *wtt;              //                   the bins' weights in ascending row order
    float *frames;                 // [B][T][n_fft]     workspace: windowed frame gradients
    float *dwav;                   // [B][L]
    int tf;                        // frames per workgroup
};

__device__ __forceinline__ int mel_row_len(const MelArgs &a, int b) {
    int len = a.L;
    if (a.lengths) len = min(max(a.lengths[b], 0), a.L);
    return len;
}

template <int LOGN>
__global__ __launch_bounds__(64 * MEL_BW_WAVES) void mel_bwd_frames_kernel(MelBwdArgs g) {
    constexpr int N = 1 << LOGN, M = N / 2, R = M / 64, H = M / 2;
    const MelArgs &a = g.f;
    extern __shared__ __attribute__((aligned(16))) unsigned char mel_bw_smem[];
    const int ks4 = (a.kstride + 3) & ~3;
    float2 *tw = reinterpret_cast<float2 *>(mel_bw_smem);                    // [M]
    float2 *twn = tw + M;                                                    // [M + 2] (kmax used)
    float2 *bufs = twn + M + 2;                                              // [MEL_BW_WAVES][2][M]
    float *mag = reinterpret_cast<float *>(bufs + MEL_BW_WAVES * 2 * M);     // [MEL_BW_WAVES][ks4]
    float *dacc = mag + MEL_BW_WAVES * ks4;                                  // [MEL_BW_WAVES][128]
    int4 *rows = reinterpret_cast<int4 *>(dacc + MEL_BW_WAVES * 128);        // [num_mels]
    float *wts = reinterpret_cast<float *>(rows + a.num_mels);               // [nw]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * g.tf;
    const int len = mel_row_len(a, b);
    const int Tb = min(mel_frames_of(len, N, a.hop, a.pad), a.T);
    if (t0 >= Tb) return;                 // frames behind the row's last one are the constant 0: they contribute nothing
    for (int i = tid; i < M; i += 64 * MEL_BW_WAVES) tw[i] = a.twm[i];
    for (int i = tid; i < a.kmax; i += 64 * MEL_BW_WAVES) twn[i] = a.twn[i];
    for (int i = tid; i < a.num_mels; i += 64 * MEL_BW_WAVES) rows[i] = a.rows[i];
    for (int i = tid; i < a.nw; i += 64 * MEL_BW_WAVES) wts[i] = a.wts[i];
    lds_barrier();

    const float *row = a.wav + (size_t)b * a.L;
    const float *drow = g.dmel + (size_t)b * a.num_mels * a.T;
    const float2 *win = reinterpret_cast<const float2 *>(a.win);             // read at both uses: 1 to 8 KB, cache resident
    auto twl = [tw](int, int, int ps, int m) { return tw[m * ps]; };
    float *mg = mag + wave * ks4, *da = dacc + wave * 128;
#pragma unroll 1
    for (int f = wave; f < g.tf; f += MEL_BW_WAVES) {
        const int t = t0 + f;
        if (t >= Tb) break;
        float2 *x = bufs + wave * 2 * M, *y = x + M;
        // this frame's column of dmel travels while the frame is transformed
        float dm[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) dm[h] = lane + 64 * h < a.num_mels ? drow[(size_t)(lane + 64 * h) * a.T + t] : 0.f;
        const int base = t * a.hop - a.pad;
#pragma unroll 1
        for (int r = 0; r < R; ++r) {
            const int j0 = base + 2 * (lane + 64 * r);
            const float2 w = win[lane + 64 * r];
            x[fft_at(lane + 64 * r)] = make_float2(row[reflect_index(j0, len)] * w.x, row[reflect_index(j0 + 1, len)] * w.y);
        }
        wave_lds_sync();
        stockham_fft<LOGN>(x, y, twl, lane);
        // ---- magnitudes as the forward forms them; bins [kmax, kmax + 3) are the zero pad of the last row's chunk
        for (int k = lane; k < a.kmax + 3; k += 64) {
            float v = 0.f;
            if (k < a.kmax) v = mel_magnitude(mel_bin(x[fft_at(k & (M - 1))], x[fft_at((M - k) & (M - 1))], twn[k]));
            mg[k] = v;
        }
        wave_lds_sync();
        // ---- acc in the forward's order, dacc with the clip's mask (lanes along the mel rows)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = lane + 64 * h;
            if (i < a.num_mels) {
                const int4 rw = rows[i];
                const float acc = mel_project(mg + rw.x, reinterpret_cast<const float4 *>(wts + rw.z), rw.y);
                da[i] = acc >= 1e-5f ? dm[h] / acc : 0.f;
            }
        }
        wave_lds_sync();
        // ---- bins k and M - k (k = 0: DC and Nyquist): H = c X with c = dmag / mag, halved on the interior bins; packed into y as
        //      the conjugate of Z'[k] = E' + i O', E' = H[k] + conj H[M-k], O' = (H[k] - conj H[M-k]) conj W^k
        auto coef = [&](int k) {
            if (k >= a.kmax) return 0.f;
            const int4 cl = g.cols[k];
            const float *w = g.wtt + cl.z;
            float s = 0.f;
            for (int i = 0; i < cl.y; ++i) s = fmaf(w[i], da[cl.x + i], s);
            return s / mg[k];
        };
#pragma unroll 1
        for (int k = lane; k <= H; k += 64) {
            const int k2 = M - k;
            const float2 wk = twn[min(k, a.kmax - 1)];        // (k >= kmax: M - k >= kmax too, both coefficients are 0)
            const RealSplit sp = real_split(x[fft_at(k & (M - 1))], x[fft_at(k2 & (M - 1))], wk);
            const float half = k == 0 ? 1.f : 0.5f;
            const float ck = half * coef(k), cm = half * coef(k2);
            float2 sk = make_float2(ck * (sp.e.x + sp.wo.x), ck * (sp.e.y + sp.wo.y));            // X[k] = E + W^k O
            float2 sm = make_float2(cm * (sp.e.x - sp.wo.x), -cm * (sp.e.y - sp.wo.y));           // X[M-k] = conj(E - W^k O)
            if (k == 0) { sk.y = 0.f; sm.y = 0.f; }
            const float epr = sk.x + sm.x, epi = sk.y - sm.y, dr = sk.x - sm.x, di = sk.y + sm.y;
            const float opr = dr * wk.x + di * wk.y, opi = di * wk.x - dr * wk.y;
            y[fft_at(k & (M - 1))] = make_float2(epr - opi, -(epi + opr));                        // conj Z'[k]
            if (k != 0 && k2 != k) y[fft_at(k2)] = make_float2(epr + opi, -(opr - epi));          // conj Z'[M-k]
        }
        wave_lds_sync();
        { float2 *tmp = x; x = y; y = tmp; }
        stockham_fft<LOGN>(x, y, twl, lane);
        // g[2m] + i g[2m+1] = conj(fft(conj Z'))[m]; windowed, stored as frame t of the workspace
        float2 *fo = reinterpret_cast<float2 *>(g.frames + ((size_t)b * a.T + t) * N);
#pragma unroll 1
        for (int r = 0; r < R; ++r) {
            const float2 z = x[fft_at(lane + 64 * r)], w = win[lane + 64 * r];
            fo[lane + 64 * r] = make_float2(z.x * w.x, -z.y * w.y);
        }
        wave_lds_sync();                  // the next frame overwrites this wave's buffers
    }
}

// what padded position q of a row collects from its frames fr [Tb][n], in ascending t, added to s
__device__ __forceinline__ float mel_bwd_collect(float s, const float *fr, int q, int pad, int hop, int n, int Tb) {
    const int p = q + pad;
    const int tlo = p >= n ? (p - n) / hop + 1 : 0, thi = min(Tb - 1, p / hop);
    for (int t = tlo; t <= thi; ++t) s += fr[(size_t)t * n + (p - t * hop)];
    return s;
}

__global__ __launch_bounds__(256) void mel_bwd_gather_kernel(MelBwdArgs g, int n) {
    const MelArgs &a = g.f;
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= a.L) return;
    const int len = mel_row_len(a, b);
    const int Tb = min(mel_frames_of(len, n, a.hop, a.pad), a.T);
    float s = 0.f;
    if (j < len && Tb > 0) {
        const float *fr = g.frames + (size_t)b * a.T * n;
        s = mel_bwd_collect(s, fr, j, a.pad, a.hop, n, Tb);
        if (j >= 1 && j <= a.pad) s = mel_bwd_collect(s, fr, -j, a.pad, a.hop, n, Tb);
        const int q = 2 * (len - 1) - j;
        if (q > len - 1 && q <= len - 1 + a.pad) s = mel_bwd_collect(s, fr, q, a.pad, a.hop, n, Tb);
    }
    g.dwav[(size_t)b * a.L + j] = s;
}

}  // namespace gtts

using namespace gtts;

namespace {

template <int LOGN>
hipError_t mel_bwd_launch(const MelBwdArgs &g, size_t smem, hipStream_t st) {
    const hipError_t e = raise_dyn_lds<&mel_bwd_frames_kernel<LOGN>>(smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mel_bwd_frames_kernel<LOGN>, dim3((unsigned)((g.f.T + g.tf - 1) / g.tf), (unsigned)g.f.B), dim3(64 * MEL_BW_WAVES),
                       smem, st, g);
    return hipGetLastError();
}

// frames per workgroup: 4 (a frame per wave) unless tiles of 8 still give the chip's 256 CUs eight workgroups each.  Measured (DESIGN
// 4.7.1, us per call, tiles of 4 / 8 / 16): 512 frames 18.9 / 29.5 / 52.0, 2080 frames 26.4 / 34.8 / 54.9, 16384 frames - / 115 / 129.
int mel_bwd_tile(int B, int T) {
#ifdef GTTS_MEL_BWD_TF                // measurement builds: a fixed tile
    return GTTS_MEL_BWD_TF;
#endif
    return (long long)B * ((T + 7) / 8) >= 2048 ? 8 : 4;
}

}  // namespace

extern "C" size_t gtts_mel_backward_workspace_bytes(const gtts_mel *m, int B, int L) {
    if (!m || B <= 0 || L <= m->pad || L > 0x7fffffff - 2 * m->pad || L + 2 * m->pad < m->cfg.n_fft) return 0;
    return align256((size_t)B * mel_frames_of(L, m->cfg.n_fft, m->cfg.hop_size, m->pad) * m->cfg.n_fft * 4);
}

extern "C" int gtts_mel_backward(const gtts_mel *m, const void *packed, const float *wav, const int *lengths, const float *dmel, float *dwav,
                                 void *workspace, size_t workspace_bytes, int B, int L, gtts_stream_t stream) {
    if (!m || !packed || !wav || !dmel || !dwav || !workspace) return fail(GTTS_E_NULL, "gtts_mel_backward: null argument");
    if (B <= 0 || B > 65535) return fail(GTTS_E_SHAPE, "gtts_mel_backward: B must lie in [1, 65535] (got %d)", B);
    const int T = gtts_mel_frames(m, L);
    if (T < 0) return T;
    if (workspace_bytes < gtts_mel_backward_workspace_bytes(m, B, L)) return fail(GTTS_E_WORKSPACE, "gtts_mel_backward: workspace too small");
    const unsigned char *blob = static_cast<const unsigned char *>(packed);
    MelBwdArgs g;
    MelArgs &a = g.f;
    a.wav = wav; a.lengths = lengths; a.out = nullptr;
    a.win = reinterpret_cast<const float *>(blob + m->off_win);
    a.twm = reinterpret_cast<const float2 *>(blob + m->off_twm);
    a.twn = reinterpret_cast<const float2 *>(blob + m->off_twn);
    a.rows = reinterpret_cast<const int4 *>(blob + m->off_rows);
    a.wts = reinterpret_cast<const float *>(blob + m->off_wts);
    a.B = B; a.L = L; a.T = T; a.hop = m->cfg.hop_size; a.pad = m->pad; a.num_mels = m->cfg.num_mels;
    a.kmax = m->kmax; a.kstride = m->kstride; a.nw = m->nw;
    g.dmel = dmel;
    g.cols = reinterpret_cast<const int4 *>(blob + m->off_cols);
    g.wtt = reinterpret_cast<const float *>(blob + m->off_wtt);
    g.frames = static_cast<float *>(workspace);
    g.dwav = dwav;
    g.tf = mel_bwd_tile(B, T);
    hipStream_t st = (hipStream_t)stream;
    switch (m->logn) {
        case 8: GTTS_HIPCHK(mel_bwd_launch<8>(g, m->smem_bwd, st)); break;
        case 9: GTTS_HIPCHK(mel_bwd_launch<9>(g, m->smem_bwd, st)); break;
        case 10: GTTS_HIPCHK(mel_bwd_launch<10>(g, m->smem_bwd, st)); break;
        default: GTTS_HIPCHK(mel_bwd_launch<11>(g, m->smem_bwd, st)); break;
    }
    hipLaunchKernelGGL(mel_bwd_gather_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)B), dim3(256), 0, st, g, m->cfg.n_fft);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}
