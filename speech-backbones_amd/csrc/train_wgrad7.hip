// train_wgrad7.hip -- weight and bias gradient of the DiffVC PostNet Block's 7x7 convolution (DiffVC/model/postnet.py:15-23, trained
// by DiffVC/train_enc.py through FwdDiffusion.compute_loss):
//     dW[co][ci][ky][kx] = sum_{b,y,x} dy[b,co,y,x] * (x * mask)[b,ci,y+ky-3,x+kx-3],     db[co] = sum_{b,y,x} dy[b,co,y,x]
// as an LDS-tiled MFMA reduction over PIXELS (the frame axis, contiguous in NCHW, is the contraction index), split-bf16 (3 MFMAs
// per product, fp32 accumulation) like every other training kernel.
//
// Tiling.  The 3x3 kernel's 64 co x 64 ci x 9 tap tile (train_wgrad.hip) does not carry over: at 49 taps its accumulators are 784
// fp32 per lane at 256 lanes, beyond the 512-register file.  A workgroup here owns 64 co x 64 ci x ONE kernel row ky (7 taps): four
// waves, each a 32 co x 32 ci x 7 tap accumulator block (112 accumulator registers), two workgroups per CU.  The seven ky
// workgroups of a (co tile, ci tile, pixel slice) have consecutive ids after the XCD banding (xcd_slot), so they run on one XCD at
// the same time and their re-reads of the same dy rows and neighbouring x rows hit that XCD's L2.
//
// Staging.  With ky fixed, an output row y meets exactly one input row y + ky - 3: a chunk is one row x 64 columns, and the x tile
// needs no halo rows, only 3 columns on each side.  Per chunk the workgroup stages dy[64 co][8 blocks of 8 pixels] and
// (x * mask)[64 ci][left edge, 8 blocks, right edge] into LDS, split once into bf16 hi / lo planes (16-byte slot per 8-pixel block;
// channel strides of 9 and 11 slots: odd, so the ds_read_b128 fragment reads of a 16-lane group spread over the banks).  The
// edges hold pixels x0 - 4 .. x0 - 1 in the upper half of the left slot and x0 + 64 .. x0 + 67 in the lower half of the right
// slot, so every block has its neighbours' near dwords at fixed offsets.  LDS: 40 KiB per workgroup of the 160 KiB per CU
// (MI355X_MICROARCH), single-buffered: two barriers per chunk, the next chunk's global loads in flight behind the MFMAs, the other
// workgroup on the CU computes while one stages.
//
// Shifts of -3 .. +3 pixels.  The MFMA k-values of a lane are 8 consecutive pixels (one block); tap kx needs the block shifted by
// kx - 3 pixels.  Over the 24-element window [left | block | right] (dwords w0..w11, only w2..w9 are read) an even shift is a
// choice of dwords (w3..w6, w4..w7, w5..w8) and an odd one a choice among the seven half-shifted dwords h_k = alignbit(w[k+1],
// w[k], 16), k = 2..8: 7 v_alignbit per plane serve all seven taps (the 3x3 kernel's +-1-pixel trick, widened).  Per k-step a wave
// reads 2 ds_read_b128 (dy) + 2 ds_read_b128 + 4 ds_read_b64 (x) and issues 21 MFMAs, well inside the LDS budget of the guide.
//
// Determinism: `nslice` workgroups per (tile, ky) own fixed contiguous chunk ranges and write their partial tiles; the 3x3 kernel's
// fixed-order reduction (wgrad_reduce_kernel, 49 taps) adds the slices and writes [cout][cin][7][7] -- no atomics, and no host
// synchronisation inside the call.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/gradtts_abi.h"
#include "common.h"
#include "kernels.h"

namespace gtts {

struct Wgrad7Args {
    const float *x;        // [B][cin][H][W]
    const float *mask;     // [B][W]
    const float *dy;       // [B][cout][H][W]
    float *part;           // [nslice][tiles][49][64 co][64 ci]
    float *dbpart;         // [nslice][cout] (written by the ci-tile-0, ky-0 workgroups), or nullptr
    int B, cin, cout, H, W;
    int ncx;               // chunks per row: ceil(W / 64)
    int nchunk;            // B * H * ncx
    int nslice;
};

constexpr int W7_DY = 9;     // 16-byte slots per co: 8 blocks + 1 pad
constexpr int W7_X = 11;     // 16-byte slots per ci: left edge, 8 blocks, right edge, 1 pad
constexpr int W7_RESIDENT_WGS = 2 * 256;     // resident workgroups of conv7x7_wgrad_kernel on an MI355X: 2 per CU x 256 CUs

__global__ __launch_bounds__(256, 2) void conv7x7_wgrad_kernel(const Wgrad7Args a) {
    __shared__ __attribute__((aligned(16))) u32x4 s_dy[2][64 * W7_DY];     // [hi | lo][co][slot]
    __shared__ __attribute__((aligned(16))) u32x4 s_x[2][64 * W7_X];       // [hi | lo][ci][slot]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kg = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int ncit = a.cin / 64;
    const int tiles = ncit * (a.cout / 64);
    const int wg = xcd_slot(blockIdx.x, gridDim.x);
    const int ky = wg % 7, tile = (wg / 7) % tiles, slice = wg / (7 * tiles);
    const int co0 = (tile / ncit) * 64, ci0 = (tile % ncit) * 64;
    const size_t HW = (size_t)a.H * a.W;
    const int per = (a.nchunk + a.nslice - 1) / a.nslice;
    const int c_begin = min(a.nchunk, slice * per), c_end = min(a.nchunk, c_begin + per);
    const bool want_db = a.dbpart != nullptr && ci0 == 0 && ky == 0;

    // whole-tensor buffer descriptors (the host keeps every tensor below 2^31 bytes): loads past the end return 0
    const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.x), 0, (int)((size_t)a.B * a.cin * HW * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsd = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.dy), 0, (int)((size_t)a.B * a.cout * HW * 4), 0x00020000);

    // Items: main (channel c = item >> 3, block = item & 7) for items tid and tid + 256 (dy and x alike: the block, and with it the
    // 8 mask values, is the same for both); edges (ci = tid >> 2, side = (tid >> 1) & 1, pixel pair tid & 1).
    const int blk_t = tid & 7;
    u32x4 xr[2][2], dr[2][2];
    float er[2];
    auto issue = [&](int ch) {
        const int cx = ch % a.ncx, y = (ch / a.ncx) % a.H, b = ch / (a.ncx * a.H);
        const int x0 = cx * 64, yy = y + ky - 3;
        const int yc = min(max(yy, 0), a.H - 1);
        const int px = min(x0 + 8 * blk_t, a.W - 1);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int c = (tid >> 3) + 32 * k;
            const int ox = (int)((((size_t)b * a.cin + ci0 + c) * HW + (size_t)yc * a.W + px) * 4);
            const int od = (int)((((size_t)b * a.cout + co0 + c) * HW + (size_t)y * a.W + px) * 4);
            xr[k][0] = __builtin_amdgcn_raw_buffer_load_b128(rsx, ox, 0, 0);
            xr[k][1] = __builtin_amdgcn_raw_buffer_load_b128(rsx, ox + 16, 0, 0);
            dr[k][0] = __builtin_amdgcn_raw_buffer_load_b128(rsd, od, 0, 0);
            dr[k][1] = __builtin_amdgcn_raw_buffer_load_b128(rsd, od + 16, 0, 0);
        }
        {
            const int ci = tid >> 2, side = (tid >> 1) & 1;
            const int pe = (side ? x0 + 64 : x0 - 4) + 2 * (tid & 1);
            const float *xrow = a.x + ((size_t)b * a.cin + ci0 + ci) * HW + (size_t)yc * a.W;
            const bool rowok = yy >= 0 && yy < a.H;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int p = pe + i;
                const bool ok = rowok && p >= 0 && p < a.W;
                const int pc = min(max(p, 0), a.W - 1);
                const float t = xrow[pc] * a.mask[(size_t)b * a.W + pc];
                er[i] = ok ? t : 0.f;
            }
        }
    };

    f32x16 acc[7];
#pragma unroll
    for (int kx = 0; kx < 7; ++kx)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[kx][r] = 0.f;
    float bsum[2] = {0.f, 0.f};

    if (c_begin < c_end) issue(c_begin);
    for (int ch = c_begin; ch < c_end; ++ch) {
        const int cx = ch % a.ncx, y = (ch / a.ncx) % a.H;
        const int x0 = cx * 64, yy = y + ky - 3;
        const bool rowok = yy >= 0 && yy < a.H;
        // (the mask is read here, not prefetched: eight more registers live across the MFMAs spill the accumulators)
        float mk[8];
        const int bb = ch / (a.ncx * a.H);
#pragma unroll
        for (int i = 0; i < 8; ++i) mk[i] = a.mask[(size_t)bb * a.W + min(x0 + 8 * blk_t + i, a.W - 1)];
        __syncthreads();                    // the previous chunk's fragment reads are done
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int c = (tid >> 3) + 32 * k, p = x0 + 8 * blk_t;
            float vx[8], vd[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const unsigned wx = xr[k][i >> 2][i & 3], wd = dr[k][i >> 2][i & 3];   // (copy first: see train_wgrad.hip)
                const bool ok = p + i < a.W;
                vx[i] = (ok && rowok) ? __builtin_bit_cast(float, wx) * mk[i] : 0.f;
                vd[i] = ok ? __builtin_bit_cast(float, wd) : 0.f;
                if (want_db) bsum[k] += vd[i];
            }
            u32x4 hi, lo;
            split8(vx, hi, lo);
            s_x[0][c * W7_X + 1 + blk_t] = hi;
            s_x[1][c * W7_X + 1 + blk_t] = lo;
            split8(vd, hi, lo);
            s_dy[0][c * W7_DY + blk_t] = hi;
            s_dy[1][c * W7_DY + blk_t] = lo;
        }
        {
            const int ci = tid >> 2, side = (tid >> 1) & 1;
            __bf16 h0, l0, h1, l1;
            split_bf16(er[0], h0, l0);
            split_bf16(er[1], h1, l1);
            // left: dwords 2, 3 of slot 0 (pixels x0 - 4 .. x0 - 1); right: dwords 0, 1 of slot 9 (x0 + 64 .. x0 + 67)
            const int di = (ci * W7_X + (side ? 9 : 0)) * 4 + (side ? 0 : 2) + (tid & 1);
            reinterpret_cast<unsigned *>(s_x[0])[di] =
                (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
            reinterpret_cast<unsigned *>(s_x[1])[di] =
                (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
        }
        __syncthreads();
        if (ch + 1 < c_end) issue(ch + 1);  // in flight behind the MFMAs
        const unsigned *xh32 = reinterpret_cast<const unsigned *>(s_x[0]), *xl32 = reinterpret_cast<const unsigned *>(s_x[1]);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int blk = 2 * ks + kg;
            const int ai = (wm * 32 + l31) * W7_DY + blk;
            const bf16x8 Ah = __builtin_bit_cast(bf16x8, s_dy[0][ai]), Al = __builtin_bit_cast(bf16x8, s_dy[1][ai]);
            const int bi = (wn * 32 + l31) * W7_X + 1 + blk;
            unsigned wh[12], wl[12];      // window dwords (indices 2..9 used)
            {
                const u32x4 dh = s_x[0][bi], dl = s_x[1][bi];
                typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
                const u32x2 Lh = *reinterpret_cast<const u32x2 *>(xh32 + (bi - 1) * 4 + 2);
                const u32x2 Ll = *reinterpret_cast<const u32x2 *>(xl32 + (bi - 1) * 4 + 2);
                const u32x2 Rh = *reinterpret_cast<const u32x2 *>(xh32 + (bi + 1) * 4);
                const u32x2 Rl = *reinterpret_cast<const u32x2 *>(xl32 + (bi + 1) * 4);
                wh[2] = Lh[0]; wh[3] = Lh[1]; wl[2] = Ll[0]; wl[3] = Ll[1];
#pragma unroll
                for (int j = 0; j < 4; ++j) { wh[4 + j] = dh[j]; wl[4 + j] = dl[j]; }
                wh[8] = Rh[0]; wh[9] = Rh[1]; wl[8] = Rl[0]; wl[9] = Rl[1];
            }
            unsigned hh[9], hl[9];        // half-shifted dwords h_k = elements (2k + 1, 2k + 2), k = 2..8
#pragma unroll
            for (int k = 2; k <= 8; ++k) {
                hh[k] = __builtin_amdgcn_alignbit(wh[k + 1], wh[k], 16);
                hl[k] = __builtin_amdgcn_alignbit(wl[k + 1], wl[k], 16);
            }
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                // fragment = window elements 5 + kx .. 12 + kx
                u32x4 bh, bl;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (kx & 1) {         // even shift: dwords (5 + kx) / 2 + j
                        bh[j] = wh[(5 + kx) / 2 + j];
                        bl[j] = wl[(5 + kx) / 2 + j];
                    } else {              // odd shift: h_{(4 + kx) / 2 + j}
                        bh[j] = hh[(4 + kx) / 2 + j];
                        bl[j] = hl[(4 + kx) / 2 + j];
                    }
                }
                const bf16x8 Bh = __builtin_bit_cast(bf16x8, bh), Bl = __builtin_bit_cast(bf16x8, bl);
                acc[kx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al, Bh, acc[kx], 0, 0, 0);
                acc[kx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bl, acc[kx], 0, 0, 0);
                acc[kx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bh, acc[kx], 0, 0, 0);
            }
        }
    }
    // ---- partial tile: D[m = co][n = ci]; lane (l31 = ci, kg) holds rows (rg&3) + 8 (rg>>2) + 4 kg
    float *out = a.part + ((size_t)slice * tiles + tile) * (49 * 64 * 64) + (size_t)ky * 7 * (64 * 64);
#pragma unroll
    for (int kx = 0; kx < 7; ++kx)
#pragma unroll
        for (int rg = 0; rg < 16; ++rg) {
            const int co = wm * 32 + (rg & 3) + 8 * (rg >> 2) + 4 * kg;
            out[(kx * 64 + co) * 64 + wn * 32 + l31] = acc[kx][rg];
        }
    if (want_db) {
        // the 8 threads (blocks) of a co are consecutive lanes: fixed-order butterfly, lane 0 of each octet publishes
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            float v = bsum[k];
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            v += __shfl_xor(v, 4, 64);
            if ((tid & 7) == 0) a.dbpart[(size_t)slice * a.cout + co0 + (tid >> 3) + 32 * k] = v;
        }
    }
}

static void wgrad7_geometry(int B, int cin, int cout, int H, int W, Wgrad7Args &a) {
    a.B = B; a.cin = cin; a.cout = cout; a.H = H; a.W = W;
    a.ncx = (W + 63) / 64;
    a.nchunk = B * H * a.ncx;
    const int wgs = (cin / 64) * (cout / 64) * 7;
    // One wave of workgroups: at 256 VGPRs per lane a CU holds two of them, 512 on the chip's 256 CUs.  The grid must FIT that
    // (floor, not ceil): every workgroup runs a whole slice, so a single workgroup past the 512 resident slots runs as a second wave
    // and adds one more slice-time to the kernel.  At least four chunks (256 pixels) per workgroup.
    int nslice = W7_RESIDENT_WGS / wgs;
    nslice = std::max(1, std::min(nslice, (a.nchunk + 3) / 4));
    a.nslice = nslice;
}

}  // namespace gtts

using namespace gtts;

extern "C" size_t gtts_conv7x7_wgrad_workspace_bytes(int B, int cin, int cout, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || cin % 64 || cout % 64) return 0;
    Wgrad7Args a;
    wgrad7_geometry(B, cin, cout, H, W, a);
    return ((size_t)a.nslice * (cin / 64) * (cout / 64) * (49 * 64 * 64) + (size_t)a.nslice * cout) * sizeof(float);
}

// dw [cout][cin][7][7] and db [cout] (nullable) of y = Conv2d_7x7(x * mask, padding 3) + bias; both are overwritten
extern "C" int gtts_conv7x7_wgrad(const float *x, const float *mask, const float *dy, float *dw, float *db, void *workspace,
                                  size_t workspace_bytes, int B, int cin, int cout, int H, int W, gtts_stream_t stream) {
    if (!x || !mask || !dy || !dw || !workspace) return fail(GTTS_E_NULL, "gtts_conv7x7_wgrad: null argument");
    if (B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0) return fail(GTTS_E_SHAPE, "gtts_conv7x7_wgrad: bad shape");
    if (cin % 64 || cout % 64) return fail(GTTS_E_CONFIG, "gtts_conv7x7_wgrad: cin and cout must be multiples of 64 (got %d, %d)", cin, cout);
    if ((size_t)B * std::max(cin, cout) * H * W >= ((size_t)1 << 29))
        return fail(GTTS_E_SHAPE, "gtts_conv7x7_wgrad: tensor too large for 32-bit offsets");
    Wgrad7Args a;
    wgrad7_geometry(B, cin, cout, H, W, a);
    a.x = x; a.mask = mask; a.dy = dy;
    hipStream_t st = (hipStream_t)stream;
    return wgrad_finish("gtts_conv7x7_wgrad", a, 49, workspace, workspace_bytes, gtts_conv7x7_wgrad_workspace_bytes(B, cin, cout, H, W), dw, db, st,
                        [st](const Wgrad7Args &a, int tiles) {
                            hipLaunchKernelGGL(conv7x7_wgrad_kernel, dim3((unsigned)(tiles * 7 * a.nslice)), dim3(256), 0, st, a);
                            return hipGetLastError();
                        });
}
