// glue_train.hip -- the alignment glue of GradTTS.compute_loss between MAS and the decoder (Grad-TTS/model/tts.py:141-181; model/tts.py
// of this package), forward and backward, for training with the encoder attached:
//   frames per token + duration loss        tts.py:141-143, utils.py:42-44
//   random out_size-frame window of y and of the path, aligned prior mean mu_y = attn^T . mu_x       tts.py:146-172
//   prior loss sum 0.5 ((y - mu_y)^2 + log 2 pi) mask / (sum(mask) F)                                tts.py:178-180
// The reference composes dense ops on the 0/1 path [B, t_x, T].  A path column holds at most one 1 and a token's frames are one
// contiguous run (monotonic_align.maximum_path), so -- as in glue.hip for inference -- the matmul is a gather, the crop is an index
// shift, and the gradient w.r.t. mu_x is a segment sum over each token's run: nothing to scatter, no atomics, every sum in a fixed
// order (the same bits on every call).  All fp32 VALU; each tensor is read once and written once.
#include <hip/hip_runtime.h>

#include "../../include/gradtts_abi.h"
#include "common.h"
#include "kernels.h"

namespace gtts {

// grid (ceil(T / 256), B): idx[b, j] = the token i with path[b, i, j] != 0 (the last such i; a valid path has at most one), else -1
__global__ __launch_bounds__(256) void align_columns_kernel(const float *__restrict__ path, int *__restrict__ idx, int tx, int T) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= T) return;
    const float *p = path + (size_t)b * tx * T + j;
    int tok = -1;
    for (int i = 0; i < tx; ++i) tok = p[(size_t)i * T] != 0.f ? i : tok;
    idx[(size_t)b * T + j] = tok;
}

// grid (B): the frames of every token from idx (staged in LDS): dur[b, i] = their number (what path.sum(-1) gives: an exact integer),
// first[b, i] = the lowest of them, -1 for a token without frames
__global__ __launch_bounds__(256) void align_tokens_kernel(const int *__restrict__ idx, float *__restrict__ dur, int *__restrict__ first, int tx,
                                                           int T) {
    extern __shared__ int s_idx[];         // [T]
    const int b = blockIdx.x;
    for (int j = threadIdx.x; j < T; j += 256) s_idx[j] = idx[(size_t)b * T + j];
    __syncthreads();
    for (int i = threadIdx.x; i < tx; i += 256) {
        int n = 0, f0 = -1;
        for (int j = 0; j < T; ++j) {
            const bool hit = s_idx[j] == i;
            f0 = (hit && f0 < 0) ? j : f0;
            n += hit ? 1 : 0;
        }
        dur[(size_t)b * tx + i] = (float)n;
        first[(size_t)b * tx + i] = f0;
    }
}

// grid (B): r = logw - log(1e-8 + dur) x_mask;  partial[b] = sum_i r^2 (fixed order);  g = 2 r  (utils.py:42-44 without the normaliser)
__global__ __launch_bounds__(256) void duration_loss_kernel(const float *__restrict__ logw, const float *__restrict__ dur,
                                                            const float *__restrict__ x_mask, float *__restrict__ partial, float *__restrict__ g,
                                                            int tx) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    float sq = 0.f;
    for (int i = threadIdx.x; i < tx; i += 256) {
        const size_t e = (size_t)b * tx + i;
        const float target = (float)log((double)(1e-8f + dur[e])) * x_mask[e];
        const float r = logw[e] - target;
        sq = fmaf(r, r, sq);
        if (g) g[e] = 2.0f * r;
    }
    sq = wave_sum(sq);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) partial[b] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Output frame c of sample b is input frame start[b] + c while c < kept[b], and empty (zeros) from there on.
// grid (ceil(S / 256), ceil(F / AG_F), B): y_c = y[.., start + c], mu_y = mu_x[.., idx[start + c]] (0 for a frame without a token) and
// partial[(b, f block, c block)] = sum over the block's live elements of 0.5 ((y_c - mu_y)^2 + log 2 pi), each thread over its features
// in ascending order, then the fixed wave / workgroup tree.
constexpr int AG_F = 8;
__global__ __launch_bounds__(256) void align_gather_fwd_kernel(const float *__restrict__ mu_x, const float *__restrict__ y, const int *__restrict__ idx,
                                                               const int *__restrict__ start, const int *__restrict__ kept, float *__restrict__ y_c,
                                                               float *__restrict__ mu_y, float *__restrict__ partial, int F, int tx, int T, int S) {
    __shared__ float red[4];
    const int c = blockIdx.x * 256 + threadIdx.x, f0 = blockIdx.y * AG_F, b = blockIdx.z;
    const bool live = c < S && c < kept[b];
    const int src = live ? min(max(start[b] + c, 0), T - 1) : 0;
    const int tok = live ? idx[(size_t)b * T + src] : -1;
    float acc = 0.f;
    if (c < S) {
        const int f1 = min(F, f0 + AG_F);
        for (int f = f0; f < f1; ++f) {
            const size_t row = (size_t)b * F + f;
            const float yv = live ? y[row * T + src] : 0.f;
            const float mv = (tok >= 0 && tok < tx) ? mu_x[row * tx + tok] : 0.f;
            y_c[row * S + c] = yv;
            mu_y[row * S + c] = mv;
            if (live) {
                const float d = yv - mv;
                acc += 0.5f * (d * d + 1.8378770664093453f);
            }
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// grid (ceil(tx / 64), ceil(F / 4), B), 64 tokens x 4 features per workgroup:
//   dmu_x[b, f, i] = sum over the live output frames c of token i, ascending, of (g_mu_y + scale (mu_y - y_c))[b, f, c]
// Token i owns the input frames [first, first + dur), i.e. the output frames [first - start, first + dur - start) cut to [0, kept).
// g_mu_y nullable (no gradient arrived through mu_y); scale: one device float, g_prior / (sum(mask) F), nullable (no prior term).
__global__ __launch_bounds__(256) void align_gather_bwd_kernel(const float *__restrict__ g_mu_y, const float *__restrict__ mu_y,
                                                               const float *__restrict__ y_c, const float *__restrict__ scale,
                                                               const float *__restrict__ dur, const int *__restrict__ first,
                                                               const int *__restrict__ start, const int *__restrict__ kept,
                                                               float *__restrict__ dmu_x, int F, int tx, int S) {
    const int i = blockIdx.x * 64 + (threadIdx.x & 63), f = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (i >= tx || f >= F) return;
    const int f0 = first[(size_t)b * tx + i], n = (int)dur[(size_t)b * tx + i];
    float acc = 0.f;
    if (f0 >= 0 && n > 0) {
        const int st = start[b];
        const int c0 = max(f0 - st, 0), c1 = min(min(f0 + n - st, kept[b]), S);
        const float sc = scale ? scale[0] : 0.f;
        const size_t row = ((size_t)b * F + f) * S;
        for (int c = c0; c < c1; ++c) {
            float v = g_mu_y ? g_mu_y[row + c] : 0.f;
            if (scale) v = fmaf(sc, mu_y[row + c] - y_c[row + c], v);
            acc += v;
        }
    }
    dmu_x[((size_t)b * F + f) * tx + i] = acc;
}

}  // namespace gtts

using namespace gtts;

static bool align_dims_ok(int B, int F, int tx, int T) {
    return B > 0 && B <= 65535 && F > 0 && tx > 0 && T > 0 && (long)F <= 4l * 65535 && (long)B * tx * T < (1l << 40) &&
           (long)B * F * T < (1l << 40) && (long)B * F * tx < (1l << 40);
}

// path [B,t_x,T] (0/1, at most one 1 per column) -> idx [B,T] int32, dur [B,t_x] fp32, first [B,t_x] int32.  T <= 40960 (idx row in LDS)
extern "C" int gtts_align_index(const float *path, int *idx, float *dur, int *first, int B, int t_x, int T, gtts_stream_t stream) {
    if (!path || !idx || !dur || !first) return fail(GTTS_E_NULL, "gtts_align_index: null argument");
    if (!align_dims_ok(B, 1, t_x, T) || (long)T * 4 > 160 * 1024) return fail(GTTS_E_SHAPE, "gtts_align_index: bad shape B=%d t_x=%d T=%d", B, t_x, T);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(align_columns_kernel, dim3((T + 255) / 256, B), dim3(256), 0, st, path, idx, t_x, T);
    GTTS_HIPCHK(hipGetLastError());
    const size_t smem = (size_t)T * sizeof(int);
    if (smem > 48 * 1024) GTTS_HIPCHK(raise_dyn_lds<&align_tokens_kernel>(smem));
    hipLaunchKernelGGL(align_tokens_kernel, dim3(B), dim3(256), smem, st, idx, dur, first, t_x, T);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}

// partials [B]: sum_i (logw - log(1e-8 + dur) x_mask)^2 per sample; grad (nullable) [B,t_x] = 2 (logw - log(1e-8 + dur) x_mask)
extern "C" int gtts_duration_loss(const float *logw, const float *dur, const float *x_mask, float *partials, float *grad, int B, int t_x,
                                  gtts_stream_t stream) {
    if (!logw || !dur || !x_mask || !partials) return fail(GTTS_E_NULL, "gtts_duration_loss: null argument");
    if (B <= 0 || t_x <= 0 || (long)B * t_x >= (1l << 40)) return fail(GTTS_E_SHAPE, "gtts_duration_loss: bad shape B=%d t_x=%d", B, t_x);
    hipLaunchKernelGGL(duration_loss_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logw, dur, x_mask, partials, grad, t_x);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}

extern "C" size_t gtts_align_gather_partials(int B, int F, int S) {
    if (B <= 0 || F <= 0 || S <= 0) return 0;
    return (size_t)B * ((F + AG_F - 1) / AG_F) * ((S + 255) / 256);
}

// mu_x [B,F,t_x], y [B,F,T], idx [B,T], start / kept [B] int32 (device) -> y_c, mu_y [B,F,S], partials [gtts_align_gather_partials].
// start and kept live on the device, so the host cannot refuse their values: a kept[b] above S counts as S, a frame start[b] + c past
// T - 1 reads frame T - 1 (as the composition's clamp does).  What the host refuses is a window longer than the frame axis (S > T).
extern "C" int gtts_align_gather_forward(const float *mu_x, const float *y, const int *idx, const int *start, const int *kept, float *y_c,
                                         float *mu_y, float *partials, int B, int F, int t_x, int T, int S, gtts_stream_t stream) {
    if (!mu_x || !y || !idx || !start || !kept || !y_c || !mu_y || !partials) return fail(GTTS_E_NULL, "gtts_align_gather_forward: null argument");
    if (!align_dims_ok(B, F, t_x, T) || S <= 0 || S > T || (long)B * F * S >= (1l << 40))
        return fail(GTTS_E_SHAPE, "gtts_align_gather_forward: bad shape B=%d F=%d t_x=%d T=%d S=%d (1 <= S <= T)", B, F, t_x, T, S);
    hipLaunchKernelGGL(align_gather_fwd_kernel, dim3((S + 255) / 256, (F + AG_F - 1) / AG_F, B), dim3(256), 0, (hipStream_t)stream, mu_x, y, idx,
                       start, kept, y_c, mu_y, partials, F, t_x, T, S);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}

extern "C" int gtts_align_gather_backward(const float *g_mu_y, const float *mu_y, const float *y_c, const float *scale, const float *dur,
                                          const int *first, const int *start, const int *kept, float *dmu_x, int B, int F, int t_x, int S,
                                          gtts_stream_t stream) {
    if (!dur || !first || !start || !kept || !dmu_x || (!g_mu_y && !scale) || (scale && (!mu_y || !y_c)))
        return fail(GTTS_E_NULL, "gtts_align_gather_backward: null argument");
    if (!align_dims_ok(B, F, t_x, 1) || S <= 0 || (long)B * F * S >= (1l << 40))
        return fail(GTTS_E_SHAPE, "gtts_align_gather_backward: bad shape B=%d F=%d t_x=%d S=%d", B, F, t_x, S);
    hipLaunchKernelGGL(align_gather_bwd_kernel, dim3((t_x + 63) / 64, (F + 3) / 4, B), dim3(256), 0, (hipStream_t)stream, g_mu_y, mu_y, y_c,
                       scale, dur, first, start, kept, dmu_x, F, t_x, S);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}
