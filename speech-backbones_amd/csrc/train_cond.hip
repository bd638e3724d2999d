// train_cond.hip -- the condition path of the DiffVC decoder's training step (DiffVC/model/diffusion.py:61-106, modules.py:128-166):
//
//   condition field   The first ResnetBlock convolves cat((mean, x), condition broadcast over the mel plane).  The convolution of a plane
//                     that is constant but for the column mask is a per-sample bias field: nine values per output channel (one for the
//                     1x1 res_conv), gated by the mask column each tap reads and by the plane's borders
//                       out[b,c,h,w] = base[b,c,h,w] + sum_{kh,kw} [0 <= h+kh-1 < H][0 <= w+kw-1 < W] m[b,w+kw-1] U[b,kh,kw,c]
//                     and its gradient w.r.t. U is the same gates summed over the plane.  U = W[:, 2:] . condition is a [B, .] contraction
//                     and stays with the caller.
//   masked mean       RefBlock's tail, final_conv -> * mask -> mean, is linear: pooling first leaves a [B, 4 base] vector for the 1x1
//                     weight.  p[b,c] = sum_{h,w} y[b,c,h,w] m[b,w] / (sum_w m[b,w] H); its backward is a broadcast.
//
// All fp32 VALU, bound by the one tensor each kernel reads or writes.  One workgroup owns one (sample, channel) plane; sums are
// per-thread partials over strided pixels in fp32, combined across the workgroup in fp64 in a fixed order: no atomics, the same bits
// on every call.
#include <hip/hip_runtime.h>

#include "../../include/gradtts_abi.h"
#include "common.h"
#include "kernels.h"

namespace gtts {

// grid (C, B), 256 threads.  U [B][TAPS][C], mask [B][W], base (nullable) and out [B][C][H][W].
template <int TAPS>
__global__ __launch_bounds__(256) void cond_field_fwd_kernel(const float *__restrict__ U, const float *__restrict__ mask,
                                                              const float *__restrict__ base, float *__restrict__ out, int C, int H, int W) {
    const int c = blockIdx.x, b = blockIdx.y, HW = H * W;
    const float *mrow = mask + (size_t)b * W;
    const size_t plane = ((size_t)b * C + c) * HW;
    float u[TAPS];
#pragma unroll
    for (int k = 0; k < TAPS; ++k) u[k] = U[((size_t)b * TAPS + k) * C + c];
    for (int p = threadIdx.x; p < HW; p += 256) {
        const int h = p / W, w = p - h * W;
        float acc = base ? base[plane + p] : 0.f;
        if constexpr (TAPS == 1) {
            acc = fmaf(mrow[w], u[0], acc);
        } else {
            float mk[3];
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int wc = w + kw - 1;
                mk[kw] = (wc >= 0 && wc < W) ? mrow[wc] : 0.f;
            }
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int hr = h + kh - 1;
                if (hr < 0 || hr >= H) continue;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) acc = fmaf(mk[kw], u[kh * 3 + kw], acc);
            }
        }
        out[plane + p] = acc;
    }
}

// grid (C, B), 256 threads.  dy [B][C][H][W] -> S [B][TAPS][C]
template <int TAPS>
__global__ __launch_bounds__(256) void cond_field_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ mask,
                                                              float *__restrict__ S, int C, int H, int W) {
    __shared__ double s_red[TAPS * 256];
    const int c = blockIdx.x, b = blockIdx.y, HW = H * W;
    const float *mrow = mask + (size_t)b * W;
    const float *d = dy + ((size_t)b * C + c) * HW;
    float acc[TAPS];
#pragma unroll
    for (int k = 0; k < TAPS; ++k) acc[k] = 0.f;
    for (int p = threadIdx.x; p < HW; p += 256) {
        const int h = p / W, w = p - h * W;
        const float v = d[p];
        if constexpr (TAPS == 1) {
            acc[0] = fmaf(v, mrow[w], acc[0]);
        } else {
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int wc = w + kw - 1;
                const float g = (wc >= 0 && wc < W) ? v * mrow[wc] : 0.f;
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    const int hr = h + kh - 1;
                    acc[kh * 3 + kw] += (hr >= 0 && hr < H) ? g : 0.f;
                }
            }
        }
    }
    double r[TAPS];
#pragma unroll
    for (int k = 0; k < TAPS; ++k) r[k] = (double)acc[k];
    block_sum_n<TAPS>(r, s_red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < TAPS; ++k) S[((size_t)b * TAPS + k) * C + c] = (float)r[k];
    }
}

// grid (C, B), 256 threads.  p[b,c] = sum_{h,w} y m[w] / (sum_w m[w] H)   (an all-zero mask row divides by zero, as the composition does)
__global__ __launch_bounds__(256) void masked_mean_fwd_kernel(const float *__restrict__ y, const float *__restrict__ mask, float *__restrict__ p,
                                                               int C, int H, int W) {
    __shared__ double s_red[2 * 256];
    const int c = blockIdx.x, b = blockIdx.y, HW = H * W;
    const float *mrow = mask + (size_t)b * W;
    const float *yp = y + ((size_t)b * C + c) * HW;
    float acc = 0.f, msum = 0.f;
    for (int i = threadIdx.x; i < HW; i += 256) {
        acc = fmaf(yp[i], mrow[i % W], acc);
    }
    for (int w = threadIdx.x; w < W; w += 256) msum += mrow[w];
    double r[2] = {(double)acc, (double)msum};
    block_sum_n<2>(r, s_red);
    if (threadIdx.x == 0) p[(size_t)b * C + c] = (float)(r[0] / (r[1] * (double)H));
}

// grid (C, B), 256 threads.  dy[b,c,h,w] = dp[b,c] m[b,w] / (sum_w m[b,w] H)
__global__ __launch_bounds__(256) void masked_mean_bwd_kernel(const float *__restrict__ dp, const float *__restrict__ mask, float *__restrict__ dy,
                                                               int C, int H, int W) {
    __shared__ double s_red[256];
    const int c = blockIdx.x, b = blockIdx.y, HW = H * W;
    const float *mrow = mask + (size_t)b * W;
    float msum = 0.f;
    for (int w = threadIdx.x; w < W; w += 256) msum += mrow[w];
    double r[1] = {(double)msum};
    block_sum_n<1>(r, s_red);
    const float g = (float)((double)dp[(size_t)b * C + c] / (r[0] * (double)H));
    float *o = dy + ((size_t)b * C + c) * HW;
    for (int i = threadIdx.x; i < HW; i += 256) o[i] = g * mrow[i % W];
}

}  // namespace gtts

using namespace gtts;

// one (sample, channel) plane per workgroup: B on grid.y, the plane indexed with an int
static bool plane_dims_ok(int B, int C, int H, int W) {
    return B > 0 && B <= 65535 && C > 0 && H > 0 && W > 0 && (long)H * W < (1l << 31) && (long)B * C * H * W < (1l << 40);
}

extern "C" int gtts_cond_field_forward(const float *U, const float *mask, const float *base, float *out, int B, int C, int H, int W, int taps,
                                       gtts_stream_t stream) {
    if (!U || !mask || !out) return fail(GTTS_E_NULL, "gtts_cond_field_forward: null argument");
    if (!plane_dims_ok(B, C, H, W)) return fail(GTTS_E_SHAPE, "gtts_cond_field_forward: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
    if (taps != 1 && taps != 9) return fail(GTTS_E_CONFIG, "gtts_cond_field_forward: taps must be 9 (3x3, padding 1) or 1 (got %d)", taps);
    hipStream_t st = (hipStream_t)stream;
    if (taps == 9) hipLaunchKernelGGL(cond_field_fwd_kernel<9>, dim3(C, B), dim3(256), 0, st, U, mask, base, out, C, H, W);
    else hipLaunchKernelGGL(cond_field_fwd_kernel<1>, dim3(C, B), dim3(256), 0, st, U, mask, base, out, C, H, W);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}

extern "C" int gtts_cond_field_backward(const float *dy, const float *mask, float *S, int B, int C, int H, int W, int taps, gtts_stream_t stream) {
    if (!dy || !mask || !S) return fail(GTTS_E_NULL, "gtts_cond_field_backward: null argument");
    if (!plane_dims_ok(B, C, H, W)) return fail(GTTS_E_SHAPE, "gtts_cond_field_backward: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
    if (taps != 1 && taps != 9) return fail(GTTS_E_CONFIG, "gtts_cond_field_backward: taps must be 9 (3x3, padding 1) or 1 (got %d)", taps);
    hipStream_t st = (hipStream_t)stream;
    if (taps == 9) hipLaunchKernelGGL(cond_field_bwd_kernel<9>, dim3(C, B), dim3(256), 0, st, dy, mask, S, C, H, W);
    else hipLaunchKernelGGL(cond_field_bwd_kernel<1>, dim3(C, B), dim3(256), 0, st, dy, mask, S, C, H, W);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}

extern "C" int gtts_masked_mean_forward(const float *y, const float *mask, float *p, int B, int C, int H, int W, gtts_stream_t stream) {
    if (!y || !mask || !p) return fail(GTTS_E_NULL, "gtts_masked_mean_forward: null argument");
    if (!plane_dims_ok(B, C, H, W)) return fail(GTTS_E_SHAPE, "gtts_masked_mean_forward: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
    hipLaunchKernelGGL(masked_mean_fwd_kernel, dim3(C, B), dim3(256), 0, (hipStream_t)stream, y, mask, p, C, H, W);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}

extern "C" int gtts_masked_mean_backward(const float *dp, const float *mask, float *dy, int B, int C, int H, int W, gtts_stream_t stream) {
    if (!dp || !mask || !dy) return fail(GTTS_E_NULL, "gtts_masked_mean_backward: null argument");
    if (!plane_dims_ok(B, C, H, W)) return fail(GTTS_E_SHAPE, "gtts_masked_mean_backward: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
    hipLaunchKernelGGL(masked_mean_bwd_kernel, dim3(C, B), dim3(256), 0, (hipStream_t)stream, dp, mask, dy, C, H, W);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}
