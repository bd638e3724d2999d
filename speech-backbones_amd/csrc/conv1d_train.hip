// conv1d_train.hip -- gradients of one Conv1d layer of the shared 1-D convolution kernel (conv1d.h): what the encoders' Conv1d layers
// need under autograd (model/_train_ops.py: EncConv1d).
//   data gradient    the forward kernel itself on dy, with the weight packed transposed and tap-reversed by gtts_conv1d_pack_dgrad
//                    (W'[ci][co][t] = W[co][ci][K-1-t]; off(K-1-t) = -off(t)) -- no convolution kernel of its own
//   weight gradient  dw[co][ci][t] = sum_b sum_q dy[b,co,q] om[b,q] * x[b,ci,q+off(t)] im[b,q+off(t)],  off(t) = (t - (K-1)/2) dilation
//   bias gradient    db[co] = sum_b sum_q dy[b,co,q] om[b,q]                                              (a plain fp32 sum)
// The weight gradient is a GEMM over the positions: per tap a [cout x (B L)] . [(B L) x cin] product.  Both operands are split
// into bf16 hi + lo on load and multiplied with three v_mfma_f32_32x32x16_bf16 per step (lo.hi, hi.lo, hi.hi; fp32 accumulate), the
// split of the forward kernel and of train_wgrad.hip: the same ~2^-17 per product, at 16/3 of the rate of the fp32-input MFMA.
// Tiling: a workgroup (4 waves, 2 x 2 of 32 x 32) owns a 64 co x 64 ci tile of ONE tap and a contiguous range of 64-position chunks
// (a chunk never crosses a sample).  Partial tiles are padded with zeros on load: rows past cout / cin, positions past L, and every
// x position q + off(t) outside [0, L) -- selected, never read (the address is clamped into the sample first).
// Determinism: `nslice` workgroups per (tile, tap) each own `per` consecutive chunks and write their partial tile, in dw's layout, to
// the workspace [nslice][cout][cin][K] (+ [nslice][cout] bias partials, from the ci-tile-0, tap-0 workgroups); a second launch adds
// the slices in ascending order.  A slice past the last chunk skips the loop and still writes its zeros.  No atomics.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/gradtts_abi.h"
#include "common.h"
#include "conv1d.h"
#include "conv1d_op.h"
#include "kernels.h"

using namespace gtts;

namespace {

constexpr int WG_T = 64;                    // output tile: 64 co x 64 ci
constexpr int WG_PC = 64;                   // positions per chunk
constexpr int WG_ROWB = (WG_PC + 8) * 2;    // bytes per LDS image row: 64 bf16 + 16 bytes of padding (conflict-free 16-byte reads)
constexpr int WG_IMG = WG_T * WG_ROWB;      // one image: [64 rows][64 positions] bf16

struct W1Args {
    const float *x;          // [B][cin][L]
    const float *dy;         // [B][cout][L]
    const float *in_mask;    // [B][L] or nullptr
    const float *out_mask;   // [B][L] or nullptr
    float *part;             // [nslice][cout][cin][K]
    float *dbpart;           // [nslice][cout], or nullptr
    int B, cin, cout, L, K, dil;
    int nq;                  // chunks per sample
    int nchunk;              // B * nq
    int nslice, per;         // slices, chunks per slice
    int ncot, ncit;
};

__global__ __launch_bounds__(256) void conv1d_wgrad_kernel(const W1Args a) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * WG_IMG];       // dy hi, dy lo, x hi, x lo
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kgl = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    int wg = blockIdx.x;
    const int cot = wg % a.ncot; wg /= a.ncot;
    const int cit = wg % a.ncit; wg /= a.ncit;
    const int tap = wg % a.K;
    const int slice = wg / a.K;
    const int off = (tap - (a.K - 1) / 2) * a.dil;
    const int c0 = slice * a.per, c1 = min(c0 + a.per, a.nchunk);
    const bool want_db = a.dbpart != nullptr && cit == 0 && tap == 0;

    // staging items: (row, 8-position group); a thread's two items share the group, so they share positions and masks
    const int g8 = (tid & 7) * 8;
    const int row0 = tid >> 3;                                    // second item: row0 + 32
    const int co_a = cot * WG_T + row0, co_b = co_a + 32;
    const int ci_a = cit * WG_T + row0, ci_b = ci_a + 32;
    float rdy[2][8], rx[2][8], rom[8], rim[8];
    unsigned okq = 0, okp = 0;                                    // bit i: position i of the group lies inside the sample (q / q + off)
    auto load_chunk = [&](int c) {
        const int b = c / a.nq, q0 = (c - b * a.nq) * WG_PC + g8;
        const float *dyb = a.dy + (size_t)b * a.cout * a.L;
        const float *xb = a.x + (size_t)b * a.cin * a.L;
        const int ra = min(co_a, a.cout - 1) * a.L, rb = min(co_b, a.cout - 1) * a.L;
        const int sa = min(ci_a, a.cin - 1) * a.L, sb = min(ci_b, a.cin - 1) * a.L;
        okq = 0; okp = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = q0 + i, p = q + off;
            const bool vq = q < a.L, vp = p >= 0 && p < a.L;
            const int qc = vq ? q : 0, pc = vp ? p : 0;           // clamped into the sample: the load is unconditional, the value selected
            okq |= (vq ? 1u : 0u) << i;
            okp |= (vp ? 1u : 0u) << i;
            rdy[0][i] = dyb[ra + qc];
            rdy[1][i] = dyb[rb + qc];
            rx[0][i] = xb[sa + pc];
            rx[1][i] = xb[sb + pc];
            rom[i] = a.out_mask ? a.out_mask[(size_t)b * a.L + qc] : 1.f;
            rim[i] = a.in_mask ? a.in_mask[(size_t)b * a.L + pc] : 1.f;
        }
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float dbs[2] = {0.f, 0.f};

    if (c0 < c1) load_chunk(c0);
    for (int c = c0; c < c1; ++c) {
        lds_barrier();                          // the previous chunk's MFMAs are done with the images
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const bool dy_row = (it ? co_b : co_a) < a.cout, x_row = (it ? ci_b : ci_a) < a.cin;
            bf16x8 dh, dl, xh, xl;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float vd = (dy_row && ((okq >> i) & 1u)) ? rdy[it][i] * rom[i] : 0.f;
                const float vx = (x_row && ((okp >> i) & 1u)) ? rx[it][i] * rim[i] : 0.f;
                dbs[it] += vd;
                __bf16 h, l;
                split_bf16(vd, h, l);
                dh[i] = h; dl[i] = l;
                split_bf16(vx, h, l);
                xh[i] = h; xl[i] = l;
            }
            const int o = (row0 + it * 32) * WG_ROWB + g8 * 2;
            *reinterpret_cast<bf16x8 *>(smem + o) = dh;
            *reinterpret_cast<bf16x8 *>(smem + WG_IMG + o) = dl;
            *reinterpret_cast<bf16x8 *>(smem + 2 * WG_IMG + o) = xh;
            *reinterpret_cast<bf16x8 *>(smem + 3 * WG_IMG + o) = xl;
        }
        if (c + 1 < c1) load_chunk(c + 1);      // in flight behind this chunk's MFMAs
        lds_barrier();
#pragma unroll
        for (int ks = 0; ks < WG_PC / 16; ++ks) {
            const int oa = (wm * 32 + l31) * WG_ROWB + (ks * 16 + kgl * 8) * 2;
            const int ob = (wn * 32 + l31) * WG_ROWB + (ks * 16 + kgl * 8) * 2;
            const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(smem + oa);
            const bf16x8 al = *reinterpret_cast<const bf16x8 *>(smem + WG_IMG + oa);
            const bf16x8 bh = *reinterpret_cast<const bf16x8 *>(smem + 2 * WG_IMG + ob);
            const bf16x8 bl = *reinterpret_cast<const bf16x8 *>(smem + 3 * WG_IMG + ob);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
        }
    }

    // partial tile -> workspace, in dw's layout: C/D row (co) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column (ci) = lane & 31
    float *part = a.part + (size_t)slice * a.cout * a.cin * a.K;
    const int ci = cit * WG_T + wn * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = cot * WG_T + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kgl;
        if (co < a.cout && ci < a.cin) part[((size_t)co * a.cin + ci) * a.K + tap] = acc[r];
    }
    if (want_db) {
        float *s_db = reinterpret_cast<float *>(smem);            // [64 rows][8 groups]
        lds_barrier();                                            // every wave is done with the images
        s_db[row0 * 8 + (tid & 7)] = dbs[0];
        s_db[(row0 + 32) * 8 + (tid & 7)] = dbs[1];
        lds_barrier();
        const int co = cot * WG_T + tid;
        if (tid < WG_T && co < a.cout) {
            float s = 0.f;
#pragma unroll
            for (int g = 0; g < 8; ++g) s += s_db[tid * 8 + g];
            a.dbpart[(size_t)slice * a.cout + co] = s;
        }
    }
}

// dw / db = the slices' partials added in ascending order; element e < n: dw, n <= e < n + cout: db
__global__ __launch_bounds__(256) void conv1d_wgrad_fold_kernel(const float *__restrict__ part, const float *__restrict__ dbpart,
                                                                float *__restrict__ dw, float *__restrict__ db, size_t n, int cout,
                                                                int nslice) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) {
        float s = 0.f;
        for (int sl = 0; sl < nslice; ++sl) s += part[(size_t)sl * n + e];
        dw[e] = s;
    } else if (db != nullptr && e < n + cout) {
        const int co = (int)(e - n);
        float s = 0.f;
        for (int sl = 0; sl < nslice; ++sl) s += dbpart[(size_t)sl * cout + co];
        db[co] = s;
    }
}

// The launcher's arithmetic, in one place: gtts_conv1d_wgrad, its workspace size and gtts_conv1d_wgrad_info all read it from here.
void wgrad_plan(const gtts_conv1d *op, int B, int L, W1Args &a) {
    a.B = B; a.cin = op->cin; a.cout = op->cout; a.L = L; a.K = op->K; a.dil = op->dil;
    a.ncot = (op->cout + WG_T - 1) / WG_T;
    a.ncit = (op->cin + WG_T - 1) / WG_T;
    a.nq = (L + WG_PC - 1) / WG_PC;
    a.nchunk = B * a.nq;
    const int tiles = a.ncot * a.ncit * op->K;
    const int want = (512 + tiles - 1) / tiles;                   // two workgroups per CU, at least four chunks each
    a.nslice = std::max(1, std::min(want, (a.nchunk + 3) / 4));
    a.per = (a.nchunk + a.nslice - 1) / a.nslice;
}
size_t wgrad_ws_bytes(const W1Args &a) {
    return ((size_t)a.nslice * a.cout * a.cin * a.K + (size_t)a.nslice * a.cout) * sizeof(float);
}

// what every gradient entry refuses on the host: a handle that is no Conv1d, a bad shape, a sample beyond the forward's limits
int wgrad_check(const gtts_conv1d *op, int B, int L, const char *fn) {
    if (op->mode != 0) return fail(GTTS_E_CONFIG, "%s: Conv1d (mode 0) handles only; ConvTranspose1d has no gradient kernels", fn);
    if (B < 1 || L < 1) return fail(GTTS_E_SHAPE, "%s: bad shape B=%d L=%d", fn, B, L);
    if ((long long)B * ((L + WG_PC - 1) / WG_PC) >= (1ll << 31)) return fail(GTTS_E_SHAPE, "%s: B * ceil(L / %d) reaches 2^31", fn, WG_PC);
    C1Args c = {};
    C1Inst inst;
    c.B = B; c.Lin = L;
    return conv1d_op_plan(op, c, &inst);          // (the 2^31-byte sample limits of gtts_conv1d_forward)
}

}  // namespace

extern "C" int gtts_conv1d_pack_dgrad(const gtts_conv1d *op_t, const float *weight, void *packed, gtts_stream_t stream) {
    if (!op_t || !weight || !packed) return fail(GTTS_E_NULL, "gtts_conv1d_pack_dgrad: null argument");
    if (op_t->mode != 0) return fail(GTTS_E_CONFIG, "gtts_conv1d_pack_dgrad: Conv1d (mode 0) handles only");
    GTTS_HIPCHK(launch_pack_conv1d(weight, (unsigned char *)packed, 2, op_t->cin, op_t->cout, op_t->K, 1, 0, (hipStream_t)stream));
    return GTTS_OK;
}

extern "C" size_t gtts_conv1d_wgrad_workspace_bytes(const gtts_conv1d *op, int B, int L) {
    if (!op || wgrad_check(op, B, L, "gtts_conv1d_wgrad_workspace_bytes")) return 0;
    W1Args a = {};
    wgrad_plan(op, B, L, a);
    return wgrad_ws_bytes(a);
}

extern "C" int gtts_conv1d_wgrad_info(const gtts_conv1d *op, int B, int L, int info[6]) {
    if (!op || !info) return fail(GTTS_E_NULL, "gtts_conv1d_wgrad_info: null argument");
    const int rc = wgrad_check(op, B, L, "gtts_conv1d_wgrad_info");
    if (rc) return rc;
    W1Args a = {};
    wgrad_plan(op, B, L, a);
    int empty = 0;
    for (int s = 0; s < a.nslice; ++s) empty += (long long)s * a.per >= a.nchunk;
    info[0] = WG_T; info[1] = WG_T; info[2] = WG_PC; info[3] = a.nslice; info[4] = a.per; info[5] = empty;
    return GTTS_OK;
}

extern "C" int gtts_conv1d_wgrad(const gtts_conv1d *op, const float *x, const float *in_mask, const float *dy, const float *out_mask, float *dw,
                                 float *db, void *workspace, size_t workspace_bytes, int B, int L, gtts_stream_t stream) {
    if (!op || !x || !dy || !dw || !workspace) return fail(GTTS_E_NULL, "gtts_conv1d_wgrad: null argument");
    const int rc = wgrad_check(op, B, L, "gtts_conv1d_wgrad");
    if (rc) return rc;
    W1Args a = {};
    wgrad_plan(op, B, L, a);
    const size_t need = wgrad_ws_bytes(a);
    if (workspace_bytes < need)
        return fail(GTTS_E_WORKSPACE, "gtts_conv1d_wgrad: workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    a.x = x; a.dy = dy; a.in_mask = in_mask; a.out_mask = out_mask;
    a.part = (float *)workspace;
    a.dbpart = db ? a.part + (size_t)a.nslice * a.cout * a.cin * a.K : nullptr;
    const size_t grid = (size_t)a.ncot * a.ncit * a.K * a.nslice;
    if (grid >= (1ull << 31)) return fail(GTTS_E_SHAPE, "gtts_conv1d_wgrad: %zu workgroups", grid);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(conv1d_wgrad_kernel, dim3((unsigned)grid), dim3(256), 0, st, a);
    GTTS_HIPCHK(hipGetLastError());
    const size_t n = (size_t)a.cout * a.cin * a.K;
    hipLaunchKernelGGL(conv1d_wgrad_fold_kernel, dim3((unsigned)((n + a.cout + 255) / 256)), dim3(256), 0, st, a.part, a.dbpart, dw, db, n,
                       a.cout, a.nslice);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}
