// train_narrow.hip -- RefBlock's narrow 3x3 convolutions for the DiffVC decoder's training step (DiffVC/model/modules.py:128-157):
// block11 (1 -> 2 base), block12 (base -> 2 base), block21 (base -> 4 base) at base = 32, whose 1 or 32 input channels fit none of the
// 64-channel tiles of train.hip / train_wgrad.hip.  Semantics as gtts_conv3x3_masked:
//   forward   y[b,n,h,w] = om[b,w] (bias[n] + sum_{k,kh,kw} w[n,k,kh,kw] x[b,k,h+kh-1,w+kw-1] m[b,w+kw-1])          (om optional)
//   dgrad     dx = m * (the same convolution of dy om with the transposed, flipped weights)                             cin 32 only
//   wgrad     dw[n,k,kh,kw] = sum_{b,h,w} (dy om)[b,n,h,w] (x m)[b,k,h+kh-1,w+kw-1],  db[n] = sum (dy om)[b,n,h,w]
// All three are implicit GEMMs on v_mfma_f32_32x32x2_f32: fp32 operands, fp32 accumulation -- bit for bit a k-ordered chain of fmaf, so
// the results are fp32-grade (no bf16 split) and repeat exactly.  No LDS: the operands are single fp32 values per lane, read straight
// from global memory (one plane row per 32 lanes, or 32 rows two pixels deep; the L1 / L2 serve the 9-fold tap reuse), and a 32x32x2
// MFMA occupies the matrix pipe for 64 cycles, which covers the two or three loads that feed it.
//   forward / dgrad   A = weights [n][k], B = patches [k][pixel]: D[n][pixel] has the pixel on the lane, so every store is a row of 32
//                     consecutive pixels.  A wave owns 32 pixels and all output channels; the weights are re-laid out [tap][k][n] into
//                     the workspace by a prologue kernel of the same call, so that 32 lanes read 32 consecutive channels.
//   wgrad             A = dy [n][pixel], B = patches [pixel][k]: D[n][k] per tap.  A workgroup owns one slice of one sample's plane;
//                     its four waves share the (channel tile, tap) accumulators.  Per-slice partials go to the workspace and a second
//                     kernel sums them in slice order in fp64: no atomics.  cin 1: the nine taps are the B columns (one tile).
#include <hip/hip_runtime.h>

#include "../../include/gradtts_abi.h"
#include "common.h"
#include "kernels.h"

namespace gtts {

typedef float nv16f __attribute__((ext_vector_type(16)));

// wt[(tap kc + k) nc + n]: forward kc = cin, nc = cout, wt = w[n][k][tap]; transposed (dgrad) kc = cout, nc = cin, wt = w[k][n][8 - tap]
__global__ void narrow_pack_kernel(const float *__restrict__ w, float *__restrict__ wt, int cin, int cout, int transposed) {
    const int i = blockIdx.x * 256 + threadIdx.x, total = 9 * cin * cout;
    if (i >= total) return;
    const int kc = transposed ? cout : cin, nc = transposed ? cin : cout;
    const int n = i % nc, k = (i / nc) % kc, tap = i / (nc * kc);
    wt[i] = transposed ? w[((size_t)k * cin + n) * 9 + (8 - tap)] : w[((size_t)n * cin + k) * 9 + tap];
}

// grid (ceil(HW / 128), B), 256 threads: wave v owns pixels [blockIdx.x 128 + 32 v, + 32) and the NT 32 output channels.
// in [B][kc][H][W], im (nullable) / om (nullable) [B][W], wt [9 kc][NT 32], bias (nullable) [NT 32], out [B][NT 32][H][W]
template <int NT>
__global__ __launch_bounds__(256) void narrow_conv_kernel(const float *__restrict__ in, const float *__restrict__ im, const float *__restrict__ om,
                                                          const float *__restrict__ wt, const float *__restrict__ bias, float *__restrict__ out,
                                                          int kc, int H, int W) {
    constexpr int NC = NT * 32;
    const int lane = threadIdx.x & 63, r = lane & 31, h2 = lane >> 5, b = blockIdx.y, HW = H * W;
    const int p = blockIdx.x * 128 + (threadIdx.x >> 6) * 32 + r;
    const bool live = p < HW;
    const int ph = live ? p / W : 0, pw = live ? p - ph * W : 0;
    const float *inb = in + (size_t)b * kc * HW;
    const float *imb = im ? im + (size_t)b * W : nullptr;
    nv16f acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    const int steps = (9 * kc + 1) / 2;
    int k = h2, tap = 0;                    // this lane's k of the step: channel k of tap `tap`
    while (k >= kc) { k -= kc; ++tap; }
    for (int s = 0; s < steps; ++s) {
        const bool kv = tap < 9;
        const int kh = tap / 3, kw = tap - 3 * kh;
        const int hr = ph + kh - 1, wc = pw + kw - 1;
        const bool ok = kv && live && hr >= 0 && hr < H && wc >= 0 && wc < W;
        float bv = 0.f;
        if (ok) {
            bv = inb[(size_t)k * HW + (size_t)hr * W + wc];
            if (imb) bv *= imb[wc];
        }
        const float *wrow = wt + ((size_t)(kv ? tap * kc + k : 0)) * NC + r;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float av = kv ? wrow[t * 32] : 0.f;
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
        }
        k += 2;
        while (k >= kc) { k -= kc; ++tap; }
    }
    if (!live) return;
    const float o = om ? om[(size_t)b * W + pw] : 1.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int n = t * 32 + (e & 3) + 8 * (e >> 2) + 4 * h2;
            out[((size_t)b * NC + n) * HW + p] = (acc[t][e] + (bias ? bias[n] : 0.f)) * o;
        }
}

// grid (nslice, B), 256 threads.  Slice sl owns pixels [sl per, min(HW, (sl + 1) per)); wave v owns the tiles t = v + 4 i of the
// NCT (CIN == 1 ? 1 : 9) (channel tile, tap) tiles.  part [B][nslice][cout cin 9 + cout]
template <int CIN, int NCT>
__global__ __launch_bounds__(256) void narrow_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ im, const float *__restrict__ om,
                                                           const float *__restrict__ dy, float *__restrict__ part, int H, int W, int per) {
    constexpr int TAPS_T = CIN == 1 ? 1 : 9, TILES = NCT * TAPS_T, TPW = (TILES + 3) / 4, COUT = NCT * 32, REC = COUT * CIN * 9 + COUT;
    const int lane = threadIdx.x & 63, r = lane & 31, h2 = lane >> 5, wv = threadIdx.x >> 6;
    const int sl = blockIdx.x, b = blockIdx.y, HW = H * W;
    const int p0 = sl * per, p1 = min(HW, p0 + per);
    const float *xb = x + (size_t)b * CIN * HW, *dyb = dy + (size_t)b * COUT * HW;
    const float *imb = im ? im + (size_t)b * W : nullptr, *omb = om ? om + (size_t)b * W : nullptr;
    nv16f acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    float dbl = 0.f;
    for (int pp = p0; pp < p1; pp += 2) {
        const int q = pp + h2;
        const bool live = q < p1;
        const int qh = live ? q / W : 0, qw = live ? q - qh * W : 0;
        const float o = (live && omb) ? omb[qw] : 1.f;
        float av[NCT];
#pragma unroll
        for (int nt = 0; nt < NCT; ++nt) {
            av[nt] = live ? dyb[(size_t)(nt * 32 + r) * HW + q] * o : 0.f;
            dbl += nt == wv ? av[nt] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int t = wv + 4 * i;
            if (t >= TILES) break;                      // (wave-uniform)
            const int nt = t / TAPS_T;
            const int tap = CIN == 1 ? r : t - nt * TAPS_T, ci = CIN == 1 ? 0 : r;
            const int kh = tap / 3, kw = tap - 3 * kh;
            const int hr = qh + kh - 1, wc = qw + kw - 1;
            float bv = 0.f;
            if (live && tap < 9 && hr >= 0 && hr < H && wc >= 0 && wc < W) {
                bv = xb[(size_t)ci * HW + (size_t)hr * W + wc];
                if (imb) bv *= imb[wc];
            }
            float a = av[0];
#pragma unroll
            for (int m = 1; m < NCT; ++m) a = nt == m ? av[m] : a;
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[i], 0, 0, 0);
        }
    }
    float *rec = part + ((size_t)b * gridDim.x + sl) * REC;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int t = wv + 4 * i;
        if (t >= TILES) break;
        const int nt = t / TAPS_T;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int n = nt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h2;
            if (CIN == 1) {
                if (r < 9) rec[(size_t)n * 9 + r] = acc[i][e];
            } else {
                rec[((size_t)n * CIN + r) * 9 + (t - nt * TAPS_T)] = acc[i][e];
            }
        }
    }
    // db: lane (r, h2) holds the sum of channel wv 32 + r over the slice's pixels of parity h2
    const float other = __shfl_xor(dbl, 32, 64);
    if (wv < NCT && h2 == 0) rec[(size_t)COUT * CIN * 9 + wv * 32 + r] = dbl + other;
}

// dw [cout cin 9] and db [cout] (nullable): the sum of the nrec records in record order, in fp64
__global__ void narrow_wgrad_finish_kernel(const float *__restrict__ part, float *__restrict__ dw, float *__restrict__ db, int nrec, int ndw,
                                           int cout) {
    const int i = blockIdx.x * 256 + threadIdx.x, rec = ndw + cout;
    if (i >= rec) return;
    double t = 0.0;
    for (int s = 0; s < nrec; ++s) t += (double)part[(size_t)s * rec + i];
    if (i < ndw) dw[i] = (float)t;
    else if (db) db[i - ndw] = (float)t;
}

}  // namespace gtts

using namespace gtts;

static bool narrow_dims_ok(int B, int H, int W) {
    return B > 0 && B <= 65535 && H > 0 && W > 0 && (long)H * W < (1l << 29) && (long)B * 128 * H * W < (1l << 40);
}
static bool narrow_config_ok(int cin, int cout) { return (cin == 1 || cin == 32) && (cout == 64 || cout == 128); }
static int narrow_slices(int B, int H, int W) {
    const long hw = (long)H * W;
    return (int)std::max(1l, std::min((hw + 255) / 256, (long)((256 + B - 1) / B)));
}

// op 0: forward, 1: data gradient (the re-laid-out weights), 2: weight gradient (the per-slice partial sums); 0 for what the entry
// points refuse
extern "C" size_t gtts_conv3x3_narrow_workspace_bytes(int B, int cin, int cout, int H, int W, int op) {
    if (!narrow_dims_ok(B, H, W) || !narrow_config_ok(cin, cout) || op < 0 || op > 2 || (op == 1 && cin != 32)) return 0;
    if (op < 2) return (size_t)9 * cin * cout * sizeof(float);
    return (size_t)B * narrow_slices(B, H, W) * ((size_t)cout * cin * 9 + cout) * sizeof(float);
}

static int narrow_run(const char *fn, const float *in, const float *im, const float *om, const float *w, const float *bias, float *out,
                      void *workspace, size_t workspace_bytes, int B, int cin, int cout, int H, int W, bool transposed, hipStream_t st) {
    const size_t need = (size_t)9 * cin * cout * sizeof(float);
    if (workspace_bytes < need) return fail(GTTS_E_WORKSPACE, "%s: workspace too small: need %zu bytes, got %zu", fn, need, workspace_bytes);
    float *wt = (float *)workspace;
    hipLaunchKernelGGL(narrow_pack_kernel, dim3((9 * cin * cout + 255) / 256), dim3(256), 0, st, w, wt, cin, cout, transposed ? 1 : 0);
    const int kc = transposed ? cout : cin, nc = transposed ? cin : cout;
    const dim3 grid((unsigned)(((long)H * W + 127) / 128), B);
    if (nc == 32) hipLaunchKernelGGL(narrow_conv_kernel<1>, grid, dim3(256), 0, st, in, im, om, wt, bias, out, kc, H, W);
    else if (nc == 64) hipLaunchKernelGGL(narrow_conv_kernel<2>, grid, dim3(256), 0, st, in, im, om, wt, bias, out, kc, H, W);
    else hipLaunchKernelGGL(narrow_conv_kernel<4>, grid, dim3(256), 0, st, in, im, om, wt, bias, out, kc, H, W);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}

extern "C" int gtts_conv3x3_narrow_forward(const float *x, const float *mask, const float *omask, const float *w, const float *bias, float *y,
                                           void *workspace, size_t workspace_bytes, int B, int cin, int cout, int H, int W,
                                           gtts_stream_t stream) {
    if (!x || !mask || !w || !bias || !y || !workspace) return fail(GTTS_E_NULL, "gtts_conv3x3_narrow_forward: null argument");
    if (!narrow_dims_ok(B, H, W)) return fail(GTTS_E_SHAPE, "gtts_conv3x3_narrow_forward: bad shape B=%d H=%d W=%d", B, H, W);
    if (!narrow_config_ok(cin, cout))
        return fail(GTTS_E_CONFIG, "gtts_conv3x3_narrow_forward: cin must be 1 or 32 and cout 64 or 128 (got cin %d, cout %d)", cin, cout);
    return narrow_run("gtts_conv3x3_narrow_forward", x, mask, omask, w, bias, y, workspace, workspace_bytes, B, cin, cout, H, W, false,
                      (hipStream_t)stream);
}

extern "C" int gtts_conv3x3_narrow_dgrad(const float *dy, const float *omask, const float *mask, const float *w, float *dx, void *workspace,
                                         size_t workspace_bytes, int B, int cin, int cout, int H, int W, gtts_stream_t stream) {
    if (!dy || !mask || !w || !dx || !workspace) return fail(GTTS_E_NULL, "gtts_conv3x3_narrow_dgrad: null argument");
    if (!narrow_dims_ok(B, H, W)) return fail(GTTS_E_SHAPE, "gtts_conv3x3_narrow_dgrad: bad shape B=%d H=%d W=%d", B, H, W);
    if (cin != 32 || !narrow_config_ok(cin, cout))
        return fail(GTTS_E_CONFIG, "gtts_conv3x3_narrow_dgrad: cin must be 32 and cout 64 or 128 (got cin %d, cout %d)", cin, cout);
    return narrow_run("gtts_conv3x3_narrow_dgrad", dy, omask, mask, w, nullptr, dx, workspace, workspace_bytes, B, cin, cout, H, W, true,
                      (hipStream_t)stream);
}

extern "C" int gtts_conv3x3_narrow_wgrad(const float *x, const float *mask, const float *omask, const float *dy, float *dw, float *db,
                                         void *workspace, size_t workspace_bytes, int B, int cin, int cout, int H, int W, gtts_stream_t stream) {
    if (!x || !mask || !dy || !dw || !workspace) return fail(GTTS_E_NULL, "gtts_conv3x3_narrow_wgrad: null argument");
    if (!narrow_dims_ok(B, H, W)) return fail(GTTS_E_SHAPE, "gtts_conv3x3_narrow_wgrad: bad shape B=%d H=%d W=%d", B, H, W);
    if (!narrow_config_ok(cin, cout))
        return fail(GTTS_E_CONFIG, "gtts_conv3x3_narrow_wgrad: cin must be 1 or 32 and cout 64 or 128 (got cin %d, cout %d)", cin, cout);
    const size_t need = gtts_conv3x3_narrow_workspace_bytes(B, cin, cout, H, W, 2);
    if (workspace_bytes < need)
        return fail(GTTS_E_WORKSPACE, "gtts_conv3x3_narrow_wgrad: workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W, ns = narrow_slices(B, H, W), per = (HW + ns - 1) / ns;
    float *part = (float *)workspace;
    const dim3 grid(ns, B);
    if (cin == 1 && cout == 64) hipLaunchKernelGGL((narrow_wgrad_kernel<1, 2>), grid, dim3(256), 0, st, x, mask, omask, dy, part, H, W, per);
    else if (cin == 1) hipLaunchKernelGGL((narrow_wgrad_kernel<1, 4>), grid, dim3(256), 0, st, x, mask, omask, dy, part, H, W, per);
    else if (cout == 64) hipLaunchKernelGGL((narrow_wgrad_kernel<32, 2>), grid, dim3(256), 0, st, x, mask, omask, dy, part, H, W, per);
    else hipLaunchKernelGGL((narrow_wgrad_kernel<32, 4>), grid, dim3(256), 0, st, x, mask, omask, dy, part, H, W, per);
    GTTS_HIPCHK(hipGetLastError());
    const int ndw = cout * cin * 9;
    hipLaunchKernelGGL(narrow_wgrad_finish_kernel, dim3((ndw + cout + 255) / 256), dim3(256), 0, st, part, dw, db, B * ns, ndw, cout);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}
