// train.hip -- first kernels of the training hot path: one score-network forward + backward
// per optimiser step at [16, C, 80, 172] (Grad-TTS/train.py:105-119; Grad-TTS/model/diffusion.py:244-252,281-294).
//
//   gtts_diffusion_noising   forward_diffusion (diffusion.py:244-252): xt = (x0 e^{-c/2} + mu (1 - e^{-c/2}) + z sqrt(1 - e^{-c})) mask
//   gtts_diffusion_noising_backward   its gradient w.r.t. x0 and mu (GradTTS.compute_loss: mu comes from the encoder)
//   gtts_score_loss          loss_t (diffusion.py:281-288): sum((eps sqrt(1 - e^{-c}) + z)^2) / (sum(mask) F) and d loss / d eps
//   gtts_conv3x3_masked      y = Conv2d_3x3(x * mask) + bias      (Block.forward, diffusion.py:56-57) on the inference MFMA kernel;
//                            the data gradient Conv2d_3x3(dy, W^T flipped) [* mask] is the same call with weights packed transposed
//   gtts_conv7x7_masked, gtts_conv1x1_masked, gtts_conv_resample     the same launch setup (conv_train_launch) on the 7x7, 1x1 and
//                            Downsample / Upsample inference kernels, and gtts_*_pack / gtts_pack_batch, which pack their weights
//   gtts_conv_train_kernel_name   which kernel instance such a call runs, from the same checks, arguments and dispatch (host only)
// The weight gradients are fixed-order MFMA reductions over pixels in train_wgrad.hip and train_wgrad7.hip; GroupNorm + Mish, the
// attention core and the elementwise ops of the step are train_norm.hip, train_attn.hip and train_elem.hip.  Every tensor-sized op
// of the step, forward and backward, is a kernel of this library: model/_train_ops.py wraps the entry points in
// torch.autograd.Function, and autograd only sequences them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/gradtts_abi.h"
#include "common.h"
#include "kernels.h"

namespace gtts {

// ------------------------------------------------------------------------------------------------ elementwise
// cum = beta_min t + 0.5 (beta_max - beta_min) t^2  (get_noise cumulative, diffusion.py:219-224), per sample
__global__ void noising_kernel(const float *__restrict__ x0, const float *__restrict__ mu, const float *__restrict__ z,
                               const float *__restrict__ mask, const float *__restrict__ t, float bmin, float bmax,
                               float *__restrict__ xt, float *__restrict__ zm, int F, int T, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / ((size_t)F * T);
    const int col = (int)(i % T);
    const float tv = t[b];
    const float cum = bmin * tv + 0.5f * (bmax - bmin) * (tv * tv);
    // correctly rounded fp32 exp (through double): 1 - e^{-cum} cancels catastrophically for t -> 0 (train.py clamps t at
    // 1e-5), where a 1-ulp difference in expf changes the noise scale by percents
    const float decay = (float)exp(-0.5 * (double)cum);
    const float m = mask[b * T + col];
    const float mean = x0[i] * decay + mu[i] * (1.0f - decay);
    const float zz = z[i];
    xt[i] = (mean + zz * sqrtf(1.0f - (float)exp(-(double)cum))) * m;
    zm[i] = zz * m;
}

// gradient of the kernel above w.r.t. x0 and mu (z carries none): dx0 = d mask dxt, dmu = (1 - d) mask dxt with d = e^{-cum/2}
// evaluated by the forward kernel's own expressions (either output nullable)
__global__ void noising_backward_kernel(const float *__restrict__ dxt, const float *__restrict__ mask, const float *__restrict__ t,
                                        float bmin, float bmax, float *__restrict__ dx0, float *__restrict__ dmu, int F, int T,
                                        size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / ((size_t)F * T);
    const int col = (int)(i % T);
    const float tv = t[b];
    const float cum = bmin * tv + 0.5f * (bmax - bmin) * (tv * tv);
    const float decay = (float)exp(-0.5 * (double)cum);
    const float g = dxt[i] * mask[b * T + col];
    if (dx0) dx0[i] = g * decay;
    if (dmu) dmu[i] = g * (1.0f - decay);
}

// r = eps * sqrt(1 - e^{-cum}) + z;  partial[blk] = sum r^2 (fixed order inside a workgroup);  geps = 2 r s / denom
__global__ void score_loss_kernel(const float *__restrict__ eps, const float *__restrict__ z, const float *__restrict__ t,
                                  float bmin, float bmax, float inv_denom, float *__restrict__ partial,
                                  float *__restrict__ geps, int F, int T, size_t total) {
    __shared__ float red[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    float sq = 0.f;
    if (i < total) {
        const size_t b = i / ((size_t)F * T);
        const float tv = t[b];
        const float cum = bmin * tv + 0.5f * (bmax - bmin) * (tv * tv);
        const float s = sqrtf(1.0f - (float)exp(-(double)cum));
        const float r = eps[i] * s + z[i];
        sq = r * r;
        if (geps) geps[i] = 2.0f * r * s * inv_denom;
    }
    sq = wave_sum(sq);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace gtts

using namespace gtts;

extern "C" int gtts_diffusion_noising(const float *x0, const float *mu, const float *z, const float *mask, const float *t,
                                      float beta_min, float beta_max, float *xt, float *z_masked, int B, int F, int T,
                                      gtts_stream_t stream) {
    if (!x0 || !mu || !z || !mask || !t || !xt || !z_masked) return fail(GTTS_E_NULL, "gtts_diffusion_noising: null argument");
    if (B <= 0 || F <= 0 || T <= 0) return fail(GTTS_E_SHAPE, "gtts_diffusion_noising: bad shape");
    const size_t total = (size_t)B * F * T;
    hipLaunchKernelGGL(noising_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x0, mu, z, mask, t,
                       beta_min, beta_max, xt, z_masked, F, T, total);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}

extern "C" int gtts_diffusion_noising_backward(const float *dxt, const float *mask, const float *t, float beta_min, float beta_max,
                                               float *dx0, float *dmu, int B, int F, int T, gtts_stream_t stream) {
    if (!dxt || !mask || !t || (!dx0 && !dmu)) return fail(GTTS_E_NULL, "gtts_diffusion_noising_backward: null argument");
    if (B <= 0 || F <= 0 || T <= 0) return fail(GTTS_E_SHAPE, "gtts_diffusion_noising_backward: bad shape");
    const size_t total = (size_t)B * F * T;
    if (total >= ((size_t)1 << 39)) return fail(GTTS_E_SHAPE, "gtts_diffusion_noising_backward: bad shape");
    hipLaunchKernelGGL(noising_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dxt, mask, t,
                       beta_min, beta_max, dx0, dmu, F, T, total);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}

extern "C" size_t gtts_score_loss_partials(int B, int F, int T) { return ((size_t)B * F * T + 255) / 256; }

extern "C" int gtts_score_loss(const float *eps, const float *z_masked, const float *t, float beta_min, float beta_max,
                               float inv_denom, float *partials, float *grad_eps, int B, int F, int T, gtts_stream_t stream) {
    if (!eps || !z_masked || !t || !partials) return fail(GTTS_E_NULL, "gtts_score_loss: null argument");
    if (B <= 0 || F <= 0 || T <= 0) return fail(GTTS_E_SHAPE, "gtts_score_loss: bad shape");
    const size_t total = (size_t)B * F * T;
    hipLaunchKernelGGL(score_loss_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, eps, z_masked, t,
                       beta_min, beta_max, inv_denom, partials, grad_eps, F, T, total);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}

// ---- the launch setup of every forward / data-gradient convolution of the training path: the inference kernel of `mode` with the
// mask prologue (mask [B][Win] on the input columns) and the plain epilogue, one weight and bias for the whole batch.  x1 (nullable):
// the input is the channel concatenation of x [B,c0,..] and x1 [B,cin-c0,..], read in place; omask (nullable): [B][Wout] column mask
// multiplied into the output.  `fn`: the entry point, for the error text.  The callers have validated every argument.
// conv_train_args is that setup alone (two: the input has a second source); gtts_conv_train_kernel_name calls it without pointers.
static ConvArgs conv_train_args(const float *x, const float *x1, bool two, int c0, const float *mask, const float *omask, const void *packed,
                                const float *bias, float *y, int B, int cin, int cout, int Hin, int Win, int Hout, int Wout) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.src0 = x; a.src1 = two ? x1 : x; a.c0 = two ? c0 : cin; a.c1 = two ? cin - c0 : 0; a.cin = cin;
    a.B = B; a.Hin = Hin; a.Win = Win; a.Hout = Hout; a.Wout = Wout;
    a.mask = mask; a.T = Win; a.lvl_in = a.lvl_out = 0;
    a.pro = PRO_MASK; a.epi = EPI_PLAIN;
    a.w = (const unsigned char *)packed; a.w_bstride = 0;
    a.bias = bias; a.bias_bstride = 0;
    a.cout = cout; a.out = y; a.groups = 8; a.nsplit = 2;
    a.omask = omask;
    return a;
}

static int conv_train_launch(int mode, const char *fn, const float *x, const float *x1, int c0, const float *mask, const float *omask,
                             const void *packed, const float *bias, float *y, int B, int cin, int cout, int Hin, int Win, int Hout,
                             int Wout, gtts_stream_t stream) {
    const ConvArgs a = conv_train_args(x, x1, x1 != nullptr, c0, mask, omask, packed, bias, y, B, cin, cout, Hin, Win, Hout, Wout);
    const hipError_t e = launch_conv(mode, a, (hipStream_t)stream);
    if (e != hipSuccess) return fail(GTTS_E_HIP, "%s (cin %d, cout %d): %s", fn, cin, cout, hipGetErrorString(e));
    return GTTS_OK;
}

// ---- weight packing: gtts_<kind>_packed_bytes is the aligned blob size of the kind's CONV_* mode, gtts_<kind>_pack this call.  cin /
// cout are those of the convolution being packed; mode + 16 packs the FORWARD weight [forward cout = cin][forward cin = cout][k][k]
// transposed with flipped taps (the data-gradient convolution).  chan: cin and cout must be multiples of it (GTTS_E_CONFIG).
static size_t train_packed_bytes(int mode, int cin, int cout, int chan = 1) {
    if (cin <= 0 || cout <= 0 || cin % chan || cout % chan) return 0;
    return align256(conv_packed_bytes(mode, cin, cout));
}

static int train_pack(int mode, const char *fn, const float *w, void *packed, int cin, int cout, gtts_stream_t stream, int chan = 1) {
    if (!w || !packed) return fail(GTTS_E_NULL, "%s: null argument", fn);
    if (cin <= 0 || cout <= 0) return fail(GTTS_E_SHAPE, "%s: bad shape", fn);
    if (cin % chan || cout % chan) return fail(GTTS_E_CONFIG, "%s: cin and cout must be multiples of %d (got %d, %d)", fn, chan, cin, cout);
    GTTS_HIPCHK(launch_pack_conv(mode, w, (unsigned char *)packed, cin, cout, (hipStream_t)stream));
    return GTTS_OK;
}

// ---- 3x3 convolutions (Block: diffusion.py:56-57): the weight gradient is gtts_conv3x3_wgrad (train_wgrad.hip)
extern "C" size_t gtts_conv3x3_packed_bytes(int cin, int cout) { return train_packed_bytes(CONV_C3, cin, cout); }

extern "C" int gtts_conv3x3_pack(const float *w, void *packed, int cin, int cout, int transposed, gtts_stream_t stream) {
    return train_pack(transposed ? CONV_C3 + 16 : CONV_C3, "gtts_conv3x3_pack", w, packed, cin, cout, stream);
}

// (the shape checks of an entry point are a function of their own: gtts_conv_train_kernel_name refuses what the entry point refuses)
static int conv3x3_check(const char *fn, bool two, int c0, int B, int cin, int cout, int H, int W) {
    if (two && (c0 <= 0 || c0 >= cin || c0 % 16)) return fail(GTTS_E_SHAPE, "%s: c0 must be a multiple of 16 inside (0, cin) (got %d of %d)", fn, c0, cin);
    if (B <= 0 || cin <= 0 || cout <= 0 || H <= 0 || W <= 0) return fail(GTTS_E_SHAPE, "%s: bad shape", fn);
    if (cout % (cout > 64 ? 128 : 64) != 0) return fail(GTTS_E_SHAPE, "%s: cout must be 64 or a multiple of 128 (got %d)", fn, cout);
    return GTTS_OK;
}

// y = Conv2d_3x3(x * mask, packed W) + bias; x [B,cin,H,W], mask [B,W] (columns), y [B,cout,H,W].  cout % 64 == 0 (128 above 64).
// x1 (nullable) / c0: the input is the channel concatenation of x [B,c0,H,W] and x1 [B,cin-c0,H,W] (c0 a multiple of 16), read
// in place (torch.cat of the up path, diffusion.py:166)
// omask (nullable): [B][W] column mask multiplied into the output -- the data gradient of a masked convolution is
// conv(dy; transposed weights) * mask, and the mask rides in the epilogue instead of a second pass over dx
extern "C" int gtts_conv3x3_masked(const float *x, const float *x1, int c0, const float *mask, const float *omask, const void *packed,
                                   const float *bias, float *y, int B, int cin, int cout, int H, int W, gtts_stream_t stream) {
    if (!x || !mask || !packed || !bias || !y) return fail(GTTS_E_NULL, "gtts_conv3x3_masked: null argument");
    const int rc = conv3x3_check("gtts_conv3x3_masked", x1 != nullptr, c0, B, cin, cout, H, W);
    if (rc != GTTS_OK) return rc;
    return conv_train_launch(CONV_C3, "gtts_conv3x3_masked", x, x1, c0, mask, omask, packed, bias, y, B, cin, cout, H, W, H, W, stream);
}

// ---- 7x7 convolutions (DiffVC PostNet Block, DiffVC/model/postnet.py:15-23) on the inference CONV_C7 kernel; the weight gradient is
// gtts_conv7x7_wgrad (train_wgrad7.hip).
// Channel counts are multiples of 64 (GTTS_E_CONFIG otherwise: the kernel's 64-cout tile and the weight gradient's 64 x 64 tile);
// every tensor of a call must stay below 2^31 bytes (GTTS_E_SHAPE): the kernels address it with 32-bit byte offsets.
static int conv7x7_check(const char *fn, int B, int cin, int cout, int H, int W) {
    if (B <= 0 || cin <= 0 || cout <= 0 || H <= 0 || W <= 0) return fail(GTTS_E_SHAPE, "%s: bad shape", fn);
    if (cin % 64 || cout % 64) return fail(GTTS_E_CONFIG, "%s: cin and cout must be multiples of 64 (got %d, %d)", fn, cin, cout);
    if ((size_t)B * std::max(cin, cout) * H * W >= ((size_t)1 << 29)) return fail(GTTS_E_SHAPE, "%s: tensor too large for 32-bit offsets", fn);
    return GTTS_OK;
}

extern "C" size_t gtts_conv7x7_packed_bytes(int cin, int cout) { return train_packed_bytes(CONV_C7, cin, cout, 64); }

extern "C" int gtts_conv7x7_pack(const float *w, void *packed, int cin, int cout, int transposed, gtts_stream_t stream) {
    return train_pack(transposed ? CONV_C7 + 16 : CONV_C7, "gtts_conv7x7_pack", w, packed, cin, cout, stream, 64);
}

// y = Conv2d_7x7(x * mask, packed W, padding 3) + bias; x [B,cin,H,W], mask [B,W] (columns), bias [cout], y [B,cout,H,W];
// omask (nullable): [B][W] column mask multiplied into the output (the data gradient of the masked convolution in one pass)
extern "C" int gtts_conv7x7_masked(const float *x, const float *mask, const float *omask, const void *packed, const float *bias,
                                   float *y, int B, int cin, int cout, int H, int W, gtts_stream_t stream) {
    if (!x || !mask || !packed || !bias || !y) return fail(GTTS_E_NULL, "gtts_conv7x7_masked: null argument");
    const int rc = conv7x7_check("gtts_conv7x7_masked", B, cin, cout, H, W);
    if (rc != GTTS_OK) return rc;
    return conv_train_launch(CONV_C7, "gtts_conv7x7_masked", x, nullptr, 0, mask, omask, packed, bias, y, B, cin, cout, H, W, H, W, stream);
}

// ---- 1x1 convolutions (res_conv, to_qkv, to_out: diffusion.py:70,87-88) on the inference CONV_P1 kernel; the weight gradient is
// gtts_conv1x1_wgrad (train_wgrad.hip)
extern "C" size_t gtts_conv1x1_packed_bytes(int cin, int cout) { return train_packed_bytes(CONV_P1, cin, cout); }

extern "C" int gtts_conv1x1_pack(const float *w, void *packed, int cin, int cout, int transposed, gtts_stream_t stream) {
    return train_pack(transposed ? CONV_P1 + 16 : CONV_P1, "gtts_conv1x1_pack", w, packed, cin, cout, stream);
}

static int conv1x1_check(const char *fn, int B, int cin, int cout, int H, int W) {
    if (B <= 0 || cin <= 0 || cout <= 0 || H <= 0 || W <= 0) return fail(GTTS_E_SHAPE, "%s: bad shape", fn);
    if (cout % (cout > 64 ? 128 : 64) != 0) return fail(GTTS_E_SHAPE, "%s: cout must be 64 or a multiple of 128 (got %d)", fn, cout);
    return GTTS_OK;
}

// y = Conv2d_1x1(x * mask, packed W) + bias; x [B,cin,H,W], mask [B,W] (columns), bias [cout], y [B,cout,H,W]
extern "C" int gtts_conv1x1_masked(const float *x, const float *mask, const void *packed, const float *bias, float *y, int B,
                                   int cin, int cout, int H, int W, gtts_stream_t stream) {
    if (!x || !mask || !packed || !bias || !y) return fail(GTTS_E_NULL, "gtts_conv1x1_masked: null argument");
    const int rc = conv1x1_check("gtts_conv1x1_masked", B, cin, cout, H, W);
    if (rc != GTTS_OK) return rc;
    return conv_train_launch(CONV_P1, "gtts_conv1x1_masked", x, nullptr, 0, mask, nullptr, packed, bias, y, B, cin, cout, H, W, H, W, stream);
}

// ---- Downsample (Conv2d 3x3, stride 2, pad 1: diffusion.py:28-34) and Upsample (ConvTranspose2d 4x4, stride 2, pad 1:
// diffusion.py:19-25) of the training path on the inference kernels.  up = 0: w [cout][cin][3][3], y [B,cout,H/2,W/2];
// up = 1: w [cin][cout][4][4] (ConvTranspose2d layout), y [B,cout,2H,2W].  The data gradient of Downsample IS an Upsample call:
// a transposed 3x3 stride-2 convolution is the 4x4 one whose fourth kernel row and column are zero (same index map
// y = 2 oy - 1 + ky), so the host packs the zero-padded forward weight with up = 1.
extern "C" size_t gtts_conv_resample_packed_bytes(int cin, int cout, int up) { return train_packed_bytes(up ? CONV_UP : CONV_DN, cin, cout); }

extern "C" int gtts_conv_resample_pack(const float *w, void *packed, int cin, int cout, int up, gtts_stream_t stream) {
    return train_pack(up ? CONV_UP : CONV_DN, "gtts_conv_resample_pack", w, packed, cin, cout, stream);
}

static int resample_check(const char *fn, int B, int cin, int cout, int H, int W, int up) {
    if (B <= 0 || cin <= 0 || cout <= 0 || H <= 0 || W <= 0) return fail(GTTS_E_SHAPE, "%s: bad shape", fn);
    if (!up && ((H | W) & 1)) return fail(GTTS_E_SHAPE, "%s: Downsample needs even H and W (got %d x %d)", fn, H, W);
    if (cin % 16 != 0 || cout % (cout > 64 ? 128 : 64) != 0)
        return fail(GTTS_E_SHAPE, "%s: cin must be a multiple of 16 and cout 64 or a multiple of 128 (got %d, %d)", fn, cin, cout);
    return GTTS_OK;
}

// y = conv(x * mask) + bias; x [B,cin,H,W], mask [B,W] (columns of the INPUT).  H and W even for up = 0.
extern "C" int gtts_conv_resample(const float *x, const float *mask, const void *packed, const float *bias, float *y, int B, int cin,
                                  int cout, int H, int W, int up, gtts_stream_t stream) {
    if (!x || !mask || !packed || !bias || !y) return fail(GTTS_E_NULL, "gtts_conv_resample: null argument");
    const int rc = resample_check("gtts_conv_resample", B, cin, cout, H, W, up);
    if (rc != GTTS_OK) return rc;
    return conv_train_launch(up ? CONV_UP : CONV_DN, up ? "gtts_conv_resample (up)" : "gtts_conv_resample (down)", x, nullptr, 0, mask, nullptr,
                             packed, bias, y, B, cin, cout, H, W, up ? 2 * H : H / 2, up ? 2 * W : W / 2, stream);
}

// ---- which kernel instance a forward / data-gradient convolution of the training path runs (additive; host only, no device call):
// the shape checks of the entry point, conv_train_args without pointers, and launch_conv describing instead of launching (common.h).
// kind 0: gtts_conv3x3_masked, 1: gtts_conv1x1_masked, 2: gtts_conv7x7_masked, 3: gtts_conv_resample (`up` read for kind 3 only).
// cin / cout / H / W are those of the call asked about (a data gradient is a call with the forward's cin and cout swapped, Downsample's
// an up = 1 call on the halved plane); c0 in (0, cin): two sources (kind 0 only), 0 or cin: one.  buf receives the name, NUL-terminated.
extern "C" int gtts_conv_train_kernel_name(int kind, int B, int cin, int c0, int cout, int H, int W, int up, char *buf, size_t n) {
    const char *fn = "gtts_conv_train_kernel_name";
    if (!buf || n == 0) return fail(GTTS_E_NULL, "%s: null argument", fn);
    buf[0] = 0;
    if (kind < 0 || kind > 3) return fail(GTTS_E_CONFIG, "%s: unknown kind %d", fn, kind);
    const bool two = c0 != 0 && c0 != cin;
    if (two && kind != 0) return fail(GTTS_E_CONFIG, "%s: only the 3x3 convolution takes two sources", fn);
    int rc, mode, Ho = H, Wo = W;
    switch (kind) {
        case 0: rc = conv3x3_check(fn, two, c0, B, cin, cout, H, W); mode = CONV_C3; break;
        case 1: rc = conv1x1_check(fn, B, cin, cout, H, W); mode = CONV_P1; break;
        case 2: rc = conv7x7_check(fn, B, cin, cout, H, W); mode = CONV_C7; break;
        default:
            rc = resample_check(fn, B, cin, cout, H, W, up); mode = up ? CONV_UP : CONV_DN;
            if (rc == GTTS_OK) { Ho = up ? 2 * H : H / 2; Wo = up ? 2 * W : W / 2; }
            break;
    }
    if (rc != GTTS_OK) return rc;
    std::string name;
    const ConvArgs a = conv_train_args(nullptr, nullptr, two, c0, nullptr, nullptr, nullptr, nullptr, nullptr, B, cin, cout, H, W, Ho, Wo);
    if (launch_conv(mode, a, nullptr, &name) != hipSuccess) return fail(GTTS_E_CONFIG, "%s: no kernel instance takes cin %d, cout %d at %d x %d", fn, cin, cout, H, W);
    if (name.size() + 1 > n) return fail(GTTS_E_WORKSPACE, "%s: the name needs %zu bytes", fn, name.size() + 1);
    memcpy(buf, name.c_str(), name.size() + 1);
    return GTTS_OK;
}

// ---- all weight packs of a training step in one launch (ABI 4) ----------------------------------------------------------
// gtts_pack_batch_describe fills `desc_host` (gtts_pack_batch_desc_bytes(n) bytes of HOST memory) with one launch descriptor per
// item; the caller copies the table to the device once (the weight and blob addresses of a module do not change between steps)
// and calls gtts_pack_batch(desc_dev, n, grid_x) at the top of every step: one launch, graph-capturable, no host work.
extern "C" size_t gtts_pack_batch_desc_bytes(int n) { return n > 0 ? (size_t)n * sizeof(PackDesc) : 0; }

extern "C" int gtts_pack_batch_describe(const gtts_pack_item *items, int n, void *desc_host, int *grid_x) {
    if (!items || !desc_host || !grid_x) return fail(GTTS_E_NULL, "gtts_pack_batch_describe: null argument");
    if (n <= 0) return fail(GTTS_E_SHAPE, "gtts_pack_batch_describe: n must be positive");
    PackDesc *d = reinterpret_cast<PackDesc *>(desc_host);
    size_t mx = 0;
    for (int k = 0; k < n; ++k) {
        const gtts_pack_item &it = items[k];
        if (!it.w || !it.packed || it.cin <= 0 || it.cout <= 0) return fail(GTTS_E_SHAPE, "gtts_pack_batch_describe: bad item %d", k);
        int mode;
        switch (it.kind) {
            case 0: mode = it.transposed ? CONV_C3 + 16 : CONV_C3; break;
            case 1: mode = it.transposed ? CONV_P1 + 16 : CONV_P1; break;
            case 2: mode = CONV_DN; break;
            case 3: mode = CONV_UP; break;
            case 4: mode = CONV_UP + 16; break;       // Downsample's data gradient: the 3x3 forward weight as a zero-padded 4x4 transposed conv
            default: return fail(GTTS_E_SHAPE, "gtts_pack_batch_describe: unknown kind %d", it.kind);
        }
        memset(&d[k], 0, sizeof(PackDesc));
        pack_describe(mode, it.w, it.packed, it.cin, it.cout, &d[k]);
        mx = std::max(mx, d[k].total);
    }
    *grid_x = (int)std::min<size_t>(std::max<size_t>((mx + 1023) / 1024, 1), 256);       // ~4 element pairs per thread on the largest weight
    return GTTS_OK;
}

extern "C" int gtts_pack_batch(const void *desc_dev, int n, int grid_x, gtts_stream_t stream) {
    if (!desc_dev) return fail(GTTS_E_NULL, "gtts_pack_batch: null argument");
    if (n <= 0 || grid_x <= 0) return fail(GTTS_E_SHAPE, "gtts_pack_batch: bad sizes");
    GTTS_HIPCHK(launch_pack_batch(reinterpret_cast<const PackDesc *>(desc_dev), n, grid_x, (hipStream_t)stream));
    return GTTS_OK;
}
