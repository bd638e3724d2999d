// mel.h -- what the log-mel forward (mel.hip) and its input gradient (mel_train.hip) share (internal header): the kernels' argument
// block, the frame count of a row, the two pieces of arithmetic that decide a cell's side of the clip -- a bin's magnitude and a mel
// row's dot product, in the forward's order of operations -- and the host handle with the layout of its packed tables.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/gradtts_abi.h"
#include "spectral.h"

namespace gtts {

struct MelArgs {
    const float *wav;              // [B][L]
    const int *lengths;            // [B] or nullptr
    float *out;                    // [B][num_mels][T]
    const float *win;              // [n_fft]           window, zero-padded to n_fft
    const float2 *twm;             // [n_fft/2]         e^{-2 pi i k / (n_fft/2)}
    const float2 *twn;             // [n_fft/2 + 1]     e^{-2 pi i k / n_fft}
    const int4 *rows;              // [num_mels]        {first bin, chunks of 4 weights, offset into wts, 0}
    const float *wts;              // [nw]              the rows' weights, each row zero-padded to whole chunks
    int B, L, T, hop, pad, num_mels, kmax, kstride, nw;
};

// frames of a row of `len` samples (0 when the row cannot be reflected or holds no whole frame)
__host__ __device__ inline int mel_frames_of(int len, int n_fft, int hop, int pad) {
    if (len <= pad || len + 2 * pad < n_fft) return 0;
    return (len + 2 * pad - n_fft) / hop + 1;
}

// X[k] = E + W^k O of the packed transform (zk = Z[k], zm = Z[M - k], w = W^k)
__device__ __forceinline__ float2 mel_bin(float2 zk, float2 zm, float2 w) {
    const RealSplit sp = real_split(zk, zm, w);
    return make_float2(sp.e.x + sp.wo.x, sp.e.y + sp.wo.y);
}

// sqrt(re^2 + im^2 + 1e-9)
__device__ __forceinline__ float mel_magnitude(float2 X) { return sqrtf(X.x * X.x + X.y * X.y + 1e-9f); }

// sum_k W[i,k] mag[k] over the row's chunks of four, one fmaf chain in ascending k (mg: the row's first bin)
__device__ __forceinline__ float mel_project(const float *mg, const float4 *w4, int chunks) {
    float acc = 0.f;
    for (int c = 0; c < chunks; ++c) {
        const float4 w = w4[c];
        acc = fmaf(w.x, mg[4 * c], acc);
        acc = fmaf(w.y, mg[4 * c + 1], acc);
        acc = fmaf(w.z, mg[4 * c + 2], acc);
        acc = fmaf(w.w, mg[4 * c + 3], acc);
    }
    return acc;
}

// LDS of the backward's frame kernel: twiddles, four waves' transform buffers, magnitudes and dacc, the rows and their weights.  It
// holds the magnitudes of 4 frames where the forward holds 16, so it is smaller than the forward's image whenever kstride >= 44, and
// below 128 KB otherwise (nw <= 128 (kstride + 3)): every configuration gtts_mel_create accepts fits.
constexpr int MEL_BW_WAVES = 4;
inline size_t mel_backward_lds(int M, int kstride, int num_mels, int nw) {
    return (size_t)M * 8 + (size_t)(M + 2) * 8 + (size_t)MEL_BW_WAVES * 2 * M * 8 + (size_t)MEL_BW_WAVES * ((kstride + 3) & ~3) * 4 +
           (size_t)MEL_BW_WAVES * 128 * 4 + (size_t)num_mels * 16 + (size_t)((nw + 3) & ~3) * 4;
}

}  // namespace gtts

// host-side metadata: the configuration and the float64-computed tables, laid out as the device blob
struct gtts_mel {
    gtts_mel_cfg cfg;
    int logn, pad, kmax, kstride, nw;
    std::vector<float> fb;                  // [num_mels][n_fft/2 + 1]
    std::vector<unsigned char> image;       // the packed blob
    size_t off_win, off_twm, off_twn, off_rows, off_wts, smem;
    // the transposed filterbank of the backward (mel_train.hip), behind the forward's tables: cols[k] = {first mel row that touches
    // bin k, rows, offset into wtt, 0} for k < kmax, wtt the bins' weights in ascending row order
    size_t off_cols, off_wtt, smem_bwd;
};
