// conv1d.hip -- one layer of the shared 1-D convolution kernel (conv1d.h) behind the C ABI: the entry the per-layer tests drive.
// The vocoder (voc.hip) and the encoders (enc.hip) reach the same kernel through the same launcher; nothing here restates its geometry.
#include <hip/hip_runtime.h>

#include "../../include/gradtts_abi.h"
#include "common.h"
#include "conv1d.h"
#include "conv1d_op.h"
#include "kernels.h"

using namespace gtts;

extern "C" int gtts_conv1d_create(int mode, int cin, int cout, int K, int dilation, int S, gtts_conv1d **out) {
    if (!out) return fail(GTTS_E_NULL, "gtts_conv1d_create: null argument");
    if (mode != 0 && mode != 1) return fail(GTTS_E_CONFIG, "conv1d mode must be 0 (Conv1d) or 1 (ConvTranspose1d), got %d", mode);
    if (cin < 1 || cout < 1 || K < 1 || dilation < 1) return fail(GTTS_E_CONFIG, "conv1d needs cin, cout, k, dilation >= 1");
    if (mode == 0 && (S != 1 || K % 2 == 0))
        return fail(GTTS_E_CONFIG, "Conv1d needs an odd kernel ('same' padding) and stride 1 (k=%d, S=%d)", K, S);
    if (mode == 1 && (S < 2 || K != 2 * S || dilation != 1))
        return fail(GTTS_E_CONFIG, "ConvTranspose1d needs stride >= 2, kernel = 2 * stride and dilation 1 (k=%d, S=%d)", K, S);
    gtts_conv1d op = {mode, cin, cout, K, dilation, S};
    C1Args a = {};
    C1Inst inst;
    a.B = 1; a.Lin = 1;                  // taps, stride and halo do not depend on the call's shape: refuse them here
    const int rc = conv1d_op_plan(&op, a, &inst);
    if (rc) return rc;
    *out = new gtts_conv1d(op);
    return GTTS_OK;
}
extern "C" void gtts_conv1d_destroy(gtts_conv1d *op) { delete op; }

extern "C" size_t gtts_conv1d_packed_bytes(const gtts_conv1d *op) {
    return op ? conv1d_packed_bytes(op->mode, op->cin, op->cout, op->K, op->S) : 0;
}
extern "C" int gtts_conv1d_pack(const gtts_conv1d *op, const float *weight, void *packed, gtts_stream_t stream) {
    if (!op || !weight || !packed) return fail(GTTS_E_NULL, "gtts_conv1d_pack: null argument");
    GTTS_HIPCHK(launch_pack_conv1d(weight, (unsigned char *)packed, op->mode, op->cin, op->cout, op->K, op->S, (op->K - op->S) / 2,
                                   (hipStream_t)stream));
    return GTTS_OK;
}

static int conv1d_op_args(const gtts_conv1d *op, C1Args &a, C1Inst *inst, const void *packed, const float *bias, const float *x, float *out,
                          const float *res, const float *accsrc, int accmode, float div, float slope, const float *in_mask,
                          const float *out_mask, int B, int Lin) {
    if (B <= 0 || Lin <= 0) return fail(GTTS_E_SHAPE, "conv1d: bad shape B=%d Lin=%d", B, Lin);
    if (accmode < 0 || accmode > 2) return fail(GTTS_E_CONFIG, "conv1d: accmode must be 0, 1 or 2 (got %d)", accmode);
    a.x = x; a.out = out; a.res = res; a.accsrc = accmode ? accsrc : nullptr; a.w = (const unsigned char *)packed; a.bias = bias;
    a.B = B; a.Lin = Lin;
    a.slope = slope; a.accmode = accmode; a.div = div;
    a.in_mask = in_mask; a.out_mask = out_mask;
    return conv1d_op_plan(op, a, inst);
}

extern "C" int gtts_conv1d_forward(const gtts_conv1d *op, const void *packed, const float *bias, const float *x, float *out, const float *res,
                                   const float *accsrc, int accmode, float div, float slope, const float *in_mask, const float *out_mask,
                                   int B, int Lin, gtts_stream_t stream) {
    if (!op || !packed || !bias || !x || !out || (accmode != 0 && !accsrc)) return fail(GTTS_E_NULL, "gtts_conv1d_forward: null argument");
    C1Args a = {};
    C1Inst inst;
    const int rc = conv1d_op_args(op, a, &inst, packed, bias, x, out, res, accsrc, accmode, div, slope, in_mask, out_mask, B, Lin);
    if (rc) return rc;
    const hipError_t e = launch_c1(a, inst, (hipStream_t)stream);
    if (e != hipSuccess) return fail(GTTS_E_HIP, "conv1d: %s", hipGetErrorString(e));
    return GTTS_OK;
}

extern "C" int gtts_conv1d_instance(const gtts_conv1d *op, int B, int Lin, int has_res, int accmode, int has_out_mask, int info[5]) {
    if (!op || !info) return fail(GTTS_E_NULL, "gtts_conv1d_instance: null argument");
    static const float one = 1.f;        // stands for "a pointer is given": the plan looks at which pointers are null, never through them
    C1Args a = {};
    C1Inst inst;
    const int rc = conv1d_op_args(op, a, &inst, nullptr, nullptr, nullptr, nullptr, has_res ? &one : nullptr, &one, accmode, 1.f, 1.f, nullptr,
                                  has_out_mask ? &one : nullptr, B, Lin);
    if (rc) return rc;
    info[0] = inst.MT; info[1] = inst.TPS; info[2] = inst.AITER; info[3] = inst.KCH; info[4] = inst.epilogue;
    return GTTS_OK;
}
