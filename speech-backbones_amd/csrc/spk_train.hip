// spk_train.hip -- training of the DiffVC speaker encoder (DiffVC/speaker_encoder/encoder/model.py, train.py): the forward of spk.hip
// keeping what the backward needs, the backward of the LSTM stack and the head, and the GE2E loss with its gradient.  fp32 throughout on
// v_mfma_f32_16x16x4_f32; every reduction runs in a fixed order and nothing is accumulated with atomics: a call repeated gives the same bits.
//
// Forward for training: spk_proj_kernel + spk_rec_kernel<true> (spk.hip) per layer, writing into the caller's `saved` tensor
//   A [M][4H] activated gates (i, f, g, o; over the layer's G), C [M][H] cell states, Hs [M][H] hidden sequence, per layer (M = N T),
//   then hlast [N][H] and raw [N][E] (the head before the L2 norm).
// Backward, from the top layer down:
//   * spk_head_bwd_kernel / spk_lin_wgrad_kernel   L2 norm, ReLU, Linear -> d hlast, dW_lin, db_lin;
//   * spk_rec_bwd_kernel    one persistent workgroup per tile of 16 sequences walks t = T - 1 ... 0 (the forward's geometry: 8 waves, each
//                           owning 32 hidden units).  Per step the lane that owns (sequence, unit) forms dh = dHseq[t] + dh_rec, the gate
//                           gradients and dc from the saved gates and cells, writes the pre-activation gradients dz over A (-> dZ) and
//                           into an LDS tile [16][4H] (64 KB, double buffered: 128.5 KB of the CU's 160 KB, one barrier per step), then
//                           dh_rec^T [H x 16] = W_hh^T [H x 4H] dz^T [4H x 16] on the MFMA, W_hh^T streamed from L2 in fragment order
//                           with the next k block in flight.  The product's rows are hidden units, so dh_rec and the dc carry meet in
//                           the lane that owns the unit; four accumulators per row tile (one per gate: chains of 256, summed pairwise).
//   * spk_dx_kernel         dX = dZ W_ih (layers above 0): the dHseq of the layer below;
//   * spk_wgrad_kernel      [dW_ih | dW_hh] = dZ^T [X | H_prev] over slices of the M rows, H_prev[n, t] = Hs[n, t - 1] by addressing
//                           (zero at t = 0); spk_colsum_kernel the bias gradient; spk_wgrad_reduce_kernel adds the slices in ascending order.
// GE2E: ge2e_kernel, one workgroup of 1024 threads, phases separated by workgroup barriers (S U = 640 rows of 256: a launch-latency job).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/gradtts_abi.h"
#include "common.h"
#include "kernels.h"
#include "spk.h"

namespace gtts {

constexpr int SPK_ZS = SPK_G + 4;                 // LDS row stride of the dz tile in floats
constexpr int SPK_WG_MINROWS = 256;               // weight gradient: rows of M per slice, at least
constexpr int SPK_WG_MAXSLICES = 16;              //                  and at most this many slices
constexpr int SPK_WG_FLUSH = 16;                  // 16-row blocks per first-level accumulation chain (256 rows)
constexpr int GE2E_SMAX = 1024;                   // speakers per batch the loss kernel's LDS row holds

// W [4H][H] row-major -> A fragments of W^T [H][4H] in the order the backward kernels walk them:
// dst[((tile * 16 + kb) * 4 + g) * 64 + lane] = W^T[16 tile + (lane & 15)][256 g + 16 kb + 4 (lane >> 4) + j], j = 0..3
__global__ void spk_pack_wT_kernel(const float *w, float4 *dst) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 16 * SPK_KB * 4 * 64) return;
    const int lane = idx & 63, g = (idx >> 6) & 3, kb = (idx >> 8) & 15, tile = idx >> 12;
    const int u = tile * 16 + (lane & 15), k = g * SPK_H + kb * 16 + (lane >> 4) * 4;
    float4 v;
    v.x = w[(size_t)k * SPK_H + u];
    v.y = w[(size_t)(k + 1) * SPK_H + u];
    v.z = w[(size_t)(k + 2) * SPK_H + u];
    v.w = w[(size_t)(k + 3) * SPK_H + u];
    dst[idx] = v;
}

// ---- recurrence backward of one layer
struct SpkRecBwdArgs {
    const float4 *whhT;     // spk_pack_wT_kernel of W_hh
    float *A;               // [N][T][4H] in: activated gates; out: dZ
    const float *C;         // [N][T][H]
    const float *dH;        // [N][T][H] gradient of the hidden sequence, or nullptr: zero except
    const float *dhlast;    // [N][H] at t = T - 1 (top layer)
    int N, T;
};

__global__ __launch_bounds__(64 * SPK_WAVES) void spk_rec_bwd_kernel(SpkRecBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float dzs[];        // [2][SPK_TILE][SPK_ZS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sq = lane & 15, q = lane >> 4;
    const int n = blockIdx.x * SPK_TILE + sq;
    const bool valid = n < a.N;
    const size_t row = (size_t)(valid ? n : 0) * a.T;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    float dc[2][4];
    f32x4 dhr[2] = {zero, zero};
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) dc[u][r] = 0.f;
    // this wave's two row tiles of W_hh^T (units 32 wave ... 32 wave + 31)
    const float4 *wp = a.whhT + (size_t)wave * 2 * SPK_KB * 4 * 64 + lane;
    float4 wcur[8], wnxt[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) wcur[x] = wp[(((x >> 2) * SPK_KB) * 4 + (x & 3)) * 64];
    // what step t reads from memory: gates, c_{t-1}, the incoming gradient of h_t
    f32x4 gt[2][4], cc[2], cp[2], dhi[2];
    auto load_step = [&](int t, f32x4(&g)[2][4], f32x4(&cprev)[2], f32x4(&dh)[2]) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int unit = (wave * 2 + u) * 16 + q * 4;
            const float *ga = a.A + (row + t) * SPK_G + unit;
#pragma unroll
            for (int k = 0; k < 4; ++k) g[u][k] = valid ? *reinterpret_cast<const f32x4 *>(ga + k * SPK_H) : zero;
            cprev[u] = valid && t > 0 ? *reinterpret_cast<const f32x4 *>(a.C + (row + t - 1) * SPK_H + unit) : zero;
            if (a.dH) dh[u] = valid ? *reinterpret_cast<const f32x4 *>(a.dH + (row + t) * SPK_H + unit) : zero;
            else dh[u] = valid && t == a.T - 1 ? *reinterpret_cast<const f32x4 *>(a.dhlast + (size_t)n * SPK_H + unit) : zero;
        }
    };
    load_step(a.T - 1, gt, cp, dhi);
#pragma unroll
    for (int u = 0; u < 2; ++u)
        cc[u] = valid ? *reinterpret_cast<const f32x4 *>(a.C + (row + a.T - 1) * SPK_H + (wave * 2 + u) * 16 + q * 4) : zero;
#pragma unroll 1
    for (int t = a.T - 1; t >= 0; --t) {
        float *zb = dzs + (size_t)(t & 1) * SPK_TILE * SPK_ZS;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x4 dz[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float gi = gt[u][0][r], gf = gt[u][1][r], gg = gt[u][2][r], go = gt[u][3][r];
                const float tc = tanhf(cc[u][r]);
                const float dh = dhi[u][r] + dhr[u][r];
                const float d_o = dh * tc;
                const float dct = fmaf(dh * go, 1.f - tc * tc, dc[u][r]);
                const float di = dct * gg, dg = dct * gi, df = dct * cp[u][r];
                dc[u][r] = dct * gf;
                dz[0][r] = di * (gi * (1.f - gi));
                dz[1][r] = df * (gf * (1.f - gf));
                dz[2][r] = dg * (1.f - gg * gg);
                dz[3][r] = d_o * (go * (1.f - go));
            }
            const int unit = (wave * 2 + u) * 16 + q * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                *reinterpret_cast<f32x4 *>(zb + sq * SPK_ZS + k * SPK_H + unit) = dz[k];
                if (valid) *reinterpret_cast<f32x4 *>(a.A + (row + t) * SPK_G + k * SPK_H + unit) = dz[k];
            }
        }
        if (t == 0) break;
        // the next step's operands travel under this step's product
        f32x4 gn[2][4], cpn[2], dhn[2];
        load_step(t - 1, gn, cpn, dhn);
        lds_barrier();            // dz_t complete; the buffer written next was last read two steps ago, before the barrier in between
        f32x4 acc[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) acc[x] = zero;
        const float *bb = zb + sq * SPK_ZS + q * 4;
#pragma unroll 2
        for (int kb = 0; kb < SPK_KB; ++kb) {
            const int nk = (kb + 1) & (SPK_KB - 1);           // wraps into the next step
#pragma unroll
            for (int x = 0; x < 8; ++x) wnxt[x] = wp[(((x >> 2) * SPK_KB + nk) * 4 + (x & 3)) * 64];
            float4 b[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) b[g] = *reinterpret_cast<const float4 *>(bb + g * SPK_H + kb * 16);
#pragma unroll
            for (int x = 0; x < 8; ++x) acc[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(wcur[x].x, b[x & 3].x, acc[x], 0, 0, 0);
#pragma unroll
            for (int x = 0; x < 8; ++x) acc[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(wcur[x].y, b[x & 3].y, acc[x], 0, 0, 0);
#pragma unroll
            for (int x = 0; x < 8; ++x) acc[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(wcur[x].z, b[x & 3].z, acc[x], 0, 0, 0);
#pragma unroll
            for (int x = 0; x < 8; ++x) acc[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(wcur[x].w, b[x & 3].w, acc[x], 0, 0, 0);
#pragma unroll
            for (int x = 0; x < 8; ++x) wcur[x] = wnxt[x];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            dhr[u] = (acc[4 * u] + acc[4 * u + 1]) + (acc[4 * u + 2] + acc[4 * u + 3]);
            cc[u] = cp[u]; cp[u] = cpn[u]; dhi[u] = dhn[u];
#pragma unroll
            for (int k = 0; k < 4; ++k) gt[u][k] = gn[u][k];
        }
    }
}

// ---- dX [M][H] = dZ [M][4H] W_ih [4H][H], computed transposed like spk_proj_kernel: wave = 16 rows of M against 8 row tiles (128 units,
// blockIdx.y); one accumulation chain per gate (256 long), added in gate order.
__global__ __launch_bounds__(256) void spk_dx_kernel(const float4 *wihT, const float *dZ, float *dX, int M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sq = lane & 15, q = lane >> 4;
    const int m = (blockIdx.x * 4 + wave) * 16 + sq;
    const bool valid = m < M;
    const float *zrow = dZ + (size_t)(valid ? m : 0) * SPK_G + q * 4;
    const int rt0 = blockIdx.y * 8;
    const float4 *wp = wihT + (size_t)rt0 * SPK_KB * 4 * 64 + lane;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 tot[8];
#pragma unroll
    for (int tl = 0; tl < 8; ++tl) tot[tl] = zero;
    for (int g = 0; g < 4; ++g) {
        f32x4 acc[8];
#pragma unroll
        for (int tl = 0; tl < 8; ++tl) acc[tl] = zero;
        for (int kb = 0; kb < SPK_KB; ++kb) {
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid) b = *reinterpret_cast<const float4 *>(zrow + g * SPK_H + kb * 16);
            float4 w[8];
#pragma unroll
            for (int tl = 0; tl < 8; ++tl) w[tl] = wp[((tl * SPK_KB + kb) * 4 + g) * 64];
#pragma unroll
            for (int tl = 0; tl < 8; ++tl) {
                acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[tl].x, b.x, acc[tl], 0, 0, 0);
                acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[tl].y, b.y, acc[tl], 0, 0, 0);
                acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[tl].z, b.z, acc[tl], 0, 0, 0);
                acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[tl].w, b.w, acc[tl], 0, 0, 0);
            }
        }
#pragma unroll
        for (int tl = 0; tl < 8; ++tl) tot[tl] += acc[tl];
    }
    if (valid) {
        float *o = dX + (size_t)m * SPK_H + q * 4;
#pragma unroll
        for (int tl = 0; tl < 8; ++tl) *reinterpret_cast<f32x4 *>(o + (rt0 + tl) * 16) = tot[tl];
    }
}

// ---- weight gradients of one layer over one slice of the M rows: part[slice][4H][NC], NC = 16 (nxt + 16) columns -- nxt column tiles of
// X (columns >= K are zero), then the 16 of H_prev.  Wave = 128 gate rows (blockIdx.y) x 2 column tiles; A = dZ^T, B = [X | H_prev], both
// read straight from memory (the k index of the product is the row of M).  Chains of SPK_WG_FLUSH blocks are flushed into a second sum.
struct SpkWgradArgs {
    const float *dZ;        // [M][4H]
    const float *X;         // [M][K]
    const float *Hs;        // [M][H]
    float *part;            // [nsl][4H][NC]
    int M, T, K, nxt, SL;
};

__global__ __launch_bounds__(256) void spk_wgrad_kernel(SpkWgradArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sq = lane & 15, q = lane >> 4;
    const int nct = a.nxt + SPK_H / 16, NC = nct * 16;
    const int ct0 = (blockIdx.x * 4 + wave) * 2;
    if (ct0 >= nct) return;                              // (no barrier in this kernel)
    const int r0 = blockIdx.y * 128;
    const int m_begin = blockIdx.z * a.SL, m_end = min(a.M, m_begin + a.SL);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[8][2], tot[8][2];
#pragma unroll
    for (int tl = 0; tl < 8; ++tl)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[tl][c] = tot[tl][c] = zero;
    int blk = 0;
    for (int mb = m_begin; mb < m_end; mb += 16, ++blk) {
        float av[8][4], bv[2][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = mb + q * 4 + j;
            const bool ok = m < m_end;
            const float *zr = a.dZ + (size_t)(ok ? m : 0) * SPK_G + r0 + sq;
#pragma unroll
            for (int tl = 0; tl < 8; ++tl) av[tl][j] = ok ? zr[tl * 16] : 0.f;
            const int t = ok ? m % a.T : 0;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int ct = ct0 + c;
                float v = 0.f;
                if (ok && ct < nct) {
                    if (ct < a.nxt) {
                        const int col = ct * 16 + sq;
                        if (col < a.K) v = a.X[(size_t)m * a.K + col];
                    } else if (t > 0) {
                        v = a.Hs[(size_t)(m - 1) * SPK_H + (ct - a.nxt) * 16 + sq];
                    }
                }
                bv[c][j] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int tl = 0; tl < 8; ++tl)
#pragma unroll
                for (int c = 0; c < 2; ++c) acc[tl][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tl][j], bv[c][j], acc[tl][c], 0, 0, 0);
        if ((blk & (SPK_WG_FLUSH - 1)) == SPK_WG_FLUSH - 1) {
#pragma unroll
            for (int tl = 0; tl < 8; ++tl)
#pragma unroll
                for (int c = 0; c < 2; ++c) { tot[tl][c] += acc[tl][c]; acc[tl][c] = zero; }
        }
    }
    float *out = a.part + (size_t)blockIdx.z * SPK_G * NC;
#pragma unroll
    for (int tl = 0; tl < 8; ++tl)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (ct0 + c >= nct) continue;
            const f32x4 v = tot[tl][c] + acc[tl][c];
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)(r0 + tl * 16 + q * 4 + r) * NC + (ct0 + c) * 16 + sq] = v[r];
        }
}

// column sums of dZ over one slice: dbpart[slice][4H]; four interleaved chains per column, added pairwise
__global__ __launch_bounds__(256) void spk_colsum_kernel(const float *dZ, float *dbpart, int M, int SL) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    const int m_begin = blockIdx.y * SL, m_end = min(M, m_begin + SL);
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int m = m_begin;
    for (; m + 4 <= m_end; m += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += dZ[(size_t)(m + k) * SPK_G + col];
    }
    for (int k = 0; m < m_end; ++m, ++k) s[k] += dZ[(size_t)m * SPK_G + col];
    dbpart[(size_t)blockIdx.y * SPK_G + col] = (s[0] + s[1]) + (s[2] + s[3]);
}

// slices added in ascending order -> dW_ih [4H][K], dW_hh [4H][H], db_ih = db_hh [4H]
__global__ void spk_wgrad_reduce_kernel(const float *part, const float *dbpart, float *dwih, float *dwhh, float *dbih, float *dbhh, int K, int nxt,
                                        int nsl) {
    const int NC = (nxt + SPK_H / 16) * 16;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= SPK_G * NC) return;
    const int rowi = idx / NC, col = idx - rowi * NC;
    if (col < nxt * 16 && col >= K) {
        if (col == K) {                                   // (a padding column of X: this thread adds the bias gradient instead)
            float s = 0.f;
            for (int k = 0; k < nsl; ++k) s += dbpart[(size_t)k * SPK_G + rowi];
            dbih[rowi] = s;
            dbhh[rowi] = s;
        }
        return;
    }
    float s = 0.f;
    for (int k = 0; k < nsl; ++k) s += part[(size_t)k * SPK_G * NC + idx];
    if (col < nxt * 16) dwih[(size_t)rowi * K + col] = s;
    else dwhh[(size_t)rowi * SPK_H + col - nxt * 16] = s;
}
__global__ void spk_bias_reduce_kernel(const float *dbpart, float *dbih, float *dbhh, int nsl) {
    const int rowi = blockIdx.x * blockDim.x + threadIdx.x;
    if (rowi >= SPK_G) return;
    float s = 0.f;
    for (int k = 0; k < nsl; ++k) s += dbpart[(size_t)k * SPK_G + rowi];
    dbih[rowi] = s;
    dbhh[rowi] = s;
}

// ---- head backward.  e = raw / ||raw||: d raw = (d - e <e, d>) / ||raw||, through the ReLU (raw > 0), then d hlast = d pre W.
__device__ __forceinline__ float spk_block_sum256(float v, float *red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void spk_head_bwd_kernel(const float *raw, const float *d_embeds, const float *w, float *dpre, float *dhlast,
                                                           int H, int E) {
    extern __shared__ float dp[];       // [E]
    __shared__ float red[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float *r = raw + (size_t)n * E, *d = d_embeds + (size_t)n * E;
    float ss = 0.f, dot = 0.f;
    for (int j = tid; j < E; j += 256) {
        ss = fmaf(r[j], r[j], ss);
        dot = fmaf(r[j], d[j], dot);
    }
    const float norm = sqrtf(spk_block_sum256(ss, red));
    const float ed = spk_block_sum256(dot, red) / norm;            // <e, d>
    for (int j = tid; j < E; j += 256) {
        const float v = r[j] > 0.f ? (d[j] - (r[j] / norm) * ed) / norm : 0.f;
        dp[j] = v;
        dpre[(size_t)n * E + j] = v;
    }
    __syncthreads();
    for (int k = tid; k < H; k += 256) {
        float acc = 0.f;
        for (int j = 0; j < E; ++j) acc = fmaf(dp[j], w[(size_t)j * H + k], acc);
        dhlast[(size_t)n * H + k] = acc;
    }
}

// dW_lin[j][k] = sum_n dpre[n][j] hlast[n][k], db_lin[j] = sum_n dpre[n][j]; one workgroup per output row j
__global__ __launch_bounds__(256) void spk_lin_wgrad_kernel(const float *dpre, const float *hlast, float *dw, float *db, int N, int H, int E) {
    __shared__ float red[256];
    const int j = blockIdx.x, tid = threadIdx.x;
    for (int k = tid; k < H; k += 256) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int n = 0; n < N; ++n) s[n & 3] = fmaf(dpre[(size_t)n * E + j], hlast[(size_t)n * H + k], s[n & 3]);
        dw[(size_t)j * H + k] = (s[0] + s[1]) + (s[2] + s[3]);
    }
    float b = 0.f;
    for (int n = tid; n < N; n += 256) b += dpre[(size_t)n * E + j];
    b = spk_block_sum256(b, red);
    if (tid == 0) db[j] = b;
}

// ---- GE2E loss and gradient (model.py:65-137 of the reference): one workgroup.
struct Ge2eArgs {
    const float *emb;       // [S][U][E]
    const float *w, *b;     // similarity_weight, similarity_bias (device scalars)
    float *sim;             // [S U][S]
    float *loss;            // [1]
    float *d_emb, *dw, *db; // nullable
    float *sum, *cin, *ynorm, *xnorm, *dcos, *rowpart, *dcin, *g, *dsum;       // workspace
    int S, U, E;
};

__global__ __launch_bounds__(1024) void ge2e_kernel(Ge2eArgs a) {
    __shared__ float cosrow[16][GE2E_SMAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S, U = a.U, E = a.E, R = S * U;
    const float w = a.w[0], b = a.b[0];
    const float um1 = (float)(U - 1), invR = 1.f / (float)R;
    // 1: per speaker the sum over its utterances, the norm of the mean and the inclusive centroid
    for (int s = wave; s < S; s += 16) {
        float ss = 0.f;
        for (int e = lane; e < E; e += 64) {
            float t = 0.f;
            for (int u = 0; u < U; ++u) t += a.emb[((size_t)s * U + u) * E + e];
            a.sum[(size_t)s * E + e] = t;
            const float y = t / (float)U;
            ss = fmaf(y, y, ss);
        }
        const float yn = sqrtf(wave_sum(ss));
        if (lane == 0) a.ynorm[s] = yn;
        for (int e = lane; e < E; e += 64) a.cin[(size_t)s * E + e] = (a.sum[(size_t)s * E + e] / (float)U) / yn;     // (own stores)
    }
    __syncthreads();
    // 2: per row the exclusive centroid's norm, the cosines, the softmax; sim, d cos and the row's share of loss, dw, db
    for (int r = wave; r < R; r += 16) {
        const int s = r / U;
        const float *er = a.emb + (size_t)r * E, *sm = a.sum + (size_t)s * E;
        float ssx = 0.f;
        for (int e = lane; e < E; e += 64) {
            const float x = (sm[e] - er[e]) / um1;
            ssx = fmaf(x, x, ssx);
        }
        const float xn = sqrtf(wave_sum(ssx));
        if (lane == 0) a.xnorm[r] = xn;
        for (int j = 0; j < S; ++j) {
            const float *cj = a.cin + (size_t)j * E;
            float d = 0.f;
            for (int e = lane; e < E; e += 64) {
                const float ev = er[e];
                const float cv = j == s ? ((sm[e] - ev) / um1) / xn : cj[e];
                d = fmaf(ev, cv, d);
            }
            d = wave_sum(d);
            if (lane == (j & 63)) cosrow[wave][j] = d;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float mx = -INFINITY;
        for (int j = lane; j < S; j += 64) mx = fmaxf(mx, __fadd_rn(__fmul_rn(cosrow[wave][j], w), b));
        mx = wave_max(mx);
        float se = 0.f;
        for (int j = lane; j < S; j += 64) se += expf(__fadd_rn(__fmul_rn(cosrow[wave][j], w), b) - mx);
        se = wave_sum(se);
        const float lse = mx + logf(se);
        // p = exp(sim - max) / sum: normalised by the sum of the very terms it divides, so a row of p sums to one to rounding whatever
        // the bias of expf or logf (exp(sim - lse) carries the rounding of lse into every term of the row with one sign)
        float dwp = 0.f, dbp = 0.f;
        for (int j = lane; j < S; j += 64) {
            const float c = cosrow[wave][j];
            const float sv = __fadd_rn(__fmul_rn(c, w), b);
            a.sim[(size_t)r * S + j] = sv;
            const float ds = (expf(sv - mx) / se - (j == s ? 1.f : 0.f)) * invR;
            a.dcos[(size_t)r * S + j] = w * ds;
            dwp = fmaf(ds, c, dwp);
            dbp += ds;
        }
        dwp = wave_sum(dwp);
        dbp = wave_sum(dbp);
        if (lane == 0) {
            a.rowpart[3 * r] = lse - __fadd_rn(__fmul_rn(cosrow[wave][s], w), b);
            a.rowpart[3 * r + 1] = dwp;
            a.rowpart[3 * r + 2] = dbp;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();                  // the row of cosines is rewritten by the wave's next row
    }
    __syncthreads();
    // 6 (needs only phase 2): loss, dw, db in ascending row order per lane, then the fixed wave tree
    if (wave == 0) {
        float l = 0.f, gw = 0.f, gb = 0.f;
        for (int r = lane; r < R; r += 64) {
            l += a.rowpart[3 * r];
            gw += a.rowpart[3 * r + 1];
            gb += a.rowpart[3 * r + 2];
        }
        l = wave_sum(l); gw = wave_sum(gw); gb = wave_sum(gb);
        if (lane == 0) {
            a.loss[0] = l * invR;
            if (a.dw) a.dw[0] = gw;
            if (a.db) a.db[0] = gb;
        }
    }
    if (!a.d_emb) return;                                 // (uniform)
    // 3a: gradient of the inclusive centroids, rows in ascending order
    for (int idx = tid; idx < S * E; idx += 1024) {
        const int j = idx / E, e = idx - j * E;
        float acc = 0.f;
        for (int r = 0; r < R; ++r)
            if (r / U != j) acc = fmaf(a.dcos[(size_t)r * S + j], a.emb[(size_t)r * E + e], acc);
        a.dcin[idx] = acc;
    }
    // 3b: per row the gradient of (sum - e) / (U - 1) through the exclusive centroid's normalisation, already divided by U - 1
    for (int r = wave; r < R; r += 16) {
        const int s = r / U;
        const float *er = a.emb + (size_t)r * E, *sm = a.sum + (size_t)s * E;
        const float xn = a.xnorm[r], dcs = a.dcos[(size_t)r * S + s];
        float in = 0.f;
        for (int e = lane; e < E; e += 64) {
            const float cex = ((sm[e] - er[e]) / um1) / xn;
            in = fmaf(cex, dcs * er[e], in);
        }
        in = wave_sum(in);
        for (int e = lane; e < E; e += 64) {
            const float cex = ((sm[e] - er[e]) / um1) / xn;
            a.g[(size_t)r * E + e] = ((dcs * er[e] - cex * in) / xn) / um1;
        }
    }
    __syncthreads();
    // 4: gradient of each speaker's sum
    for (int s = wave; s < S; s += 16) {
        const float *cs = a.cin + (size_t)s * E, *dcn = a.dcin + (size_t)s * E;
        float in = 0.f;
        for (int e = lane; e < E; e += 64) in = fmaf(cs[e], dcn[e], in);
        in = wave_sum(in);
        const float yn = a.ynorm[s];
        for (int e = lane; e < E; e += 64) {
            float t = ((dcn[e] - cs[e] * in) / yn) / (float)U;
            for (int u = 0; u < U; ++u) t += a.g[((size_t)s * U + u) * E + e];
            a.dsum[(size_t)s * E + e] = t;
        }
    }
    __syncthreads();
    // 5: d e = sum_{j != s} d cos_j cin_j + d cos_s cex - g + d sum_s
    for (int idx = tid; idx < R * E; idx += 1024) {
        const int r = idx / E, e = idx - r * E, s = r / U;
        float acc = 0.f;
        for (int j = 0; j < S; ++j)
            if (j != s) acc = fmaf(a.dcos[(size_t)r * S + j], a.cin[(size_t)j * E + e], acc);
        const float cex = ((a.sum[(size_t)s * E + e] - a.emb[idx]) / um1) / a.xnorm[r];
        acc = fmaf(a.dcos[(size_t)r * S + s], cex, acc);
        a.d_emb[idx] = (acc - a.g[idx]) + a.dsum[(size_t)s * E + e];
    }
}

}  // namespace gtts

using namespace gtts;

// ---- layouts
struct SpkSaved {
    size_t A[8], C[8], Hs[8], hlast, raw, bytes;
};
static SpkSaved spk_saved(const gtts_spk *s, int N, int T) {
    SpkSaved v;
    const size_t rows = (size_t)N * T;
    size_t o = 0;
    for (int l = 0; l < s->cfg.layers; ++l) {
        v.A[l] = o; o += align256(rows * SPK_G * 4);
        v.C[l] = o; o += align256(rows * SPK_H * 4);
        v.Hs[l] = o; o += align256(rows * SPK_H * 4);
    }
    v.hlast = o; o += align256((size_t)N * SPK_H * 4);
    v.raw = o; o += align256((size_t)N * s->cfg.embed * 4);
    v.bytes = o;
    return v;
}
static void spk_slices(int M, int *SL, int *nsl) {
    int sl = (M + SPK_WG_MAXSLICES - 1) / SPK_WG_MAXSLICES;
    sl = (sl + 15) / 16 * 16;
    if (sl < SPK_WG_MINROWS) sl = SPK_WG_MINROWS;
    *SL = sl;
    *nsl = (M + sl - 1) / sl;
}
struct SpkTrainWs {
    size_t dH, dpre, dhlast, part, dbpart, bytes;
};
static SpkTrainWs spk_train_ws(const gtts_spk *s, int N, int T) {
    SpkTrainWs v;
    int SL, nsl;
    spk_slices(N * T, &SL, &nsl);
    size_t o = 0;
    v.dH = o; o += align256((size_t)N * T * SPK_H * 4);
    v.dpre = o; o += align256((size_t)N * s->cfg.embed * 4);
    v.dhlast = o; o += align256((size_t)N * SPK_H * 4);
    const int nxt = s->kb[0] > SPK_H / 16 ? s->kb[0] : SPK_H / 16;       // the widest layer's column tiles of X
    v.part = o; o += align256((size_t)nsl * SPK_G * (nxt + SPK_H / 16) * 16 * 4);
    v.dbpart = o; o += align256((size_t)nsl * SPK_G * 4);
    v.bytes = o;
    return v;
}
struct SpkTrainBlob {
    size_t whhT[8], wihT[8], lin_w, bytes;
};
static SpkTrainBlob spk_train_blob(const gtts_spk *s) {
    SpkTrainBlob v;
    const size_t frag = (size_t)16 * SPK_KB * 4 * 64 * 16;
    size_t o = 0;
    for (int l = 0; l < s->cfg.layers; ++l) {
        v.whhT[l] = o; o += frag;
        v.wihT[l] = o; o += l > 0 ? frag : 0;
    }
    v.lin_w = o; o += align256((size_t)s->cfg.embed * s->cfg.hidden * 4);
    v.bytes = o;
    return v;
}

extern "C" size_t gtts_spktrain_packed_bytes(const gtts_spk *s) { return s ? spk_train_blob(s).bytes : 0; }
extern "C" size_t gtts_spktrain_saved_bytes(const gtts_spk *s, int N, int T) { return s && spk_shape_ok(N, T) ? spk_saved(s, N, T).bytes : 0; }
extern "C" size_t gtts_spktrain_workspace_bytes(const gtts_spk *s, int N, int T) {
    return s && spk_shape_ok(N, T) ? spk_train_ws(s, N, T).bytes : 0;
}

extern "C" int gtts_spktrain_pack(const gtts_spk *s, const void *const *ptrs, int n, void *packed, gtts_stream_t stream) {
    if (!s || !ptrs || !packed) return fail(GTTS_E_NULL, "gtts_spktrain_pack: null argument");
    if (n != (int)s->params.size()) return fail(GTTS_E_PARAMS, "spk: expected %d parameters, got %d", (int)s->params.size(), n);
    for (int i = 0; i < n; ++i)
        if (!ptrs[i]) return fail(GTTS_E_NULL, "spk: parameter %s is null", s->params[i].name.c_str());
    hipStream_t st = (hipStream_t)stream;
    unsigned char *blob = static_cast<unsigned char *>(packed);
    const SpkTrainBlob tb = spk_train_blob(s);
    const int cnt = 16 * SPK_KB * 4 * 64;
    for (int l = 0; l < s->cfg.layers; ++l) {
        hipLaunchKernelGGL(spk_pack_wT_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, (const float *)ptrs[4 * l + 1], (float4 *)(blob + tb.whhT[l]));
        GTTS_HIPCHK(hipGetLastError());
        if (l > 0) {
            hipLaunchKernelGGL(spk_pack_wT_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, (const float *)ptrs[4 * l], (float4 *)(blob + tb.wihT[l]));
            GTTS_HIPCHK(hipGetLastError());
        }
    }
    GTTS_HIPCHK(hipMemcpyAsync(blob + tb.lin_w, ptrs[4 * s->cfg.layers], (size_t)s->cfg.embed * s->cfg.hidden * 4, hipMemcpyDeviceToDevice, st));
    return GTTS_OK;
}

extern "C" int gtts_spktrain_forward(const gtts_spk *s, const void *packed, const float *frames, int N, int T, float *embeds, void *saved,
                                      size_t saved_bytes, gtts_stream_t stream) {
    if (!s || !packed || !frames || !embeds || !saved) return fail(GTTS_E_NULL, "gtts_spktrain_forward: null argument");
    if (N < 1 || T < 1) return fail(GTTS_E_SHAPE, "gtts_spktrain_forward: bad shape N=%d T=%d", N, T);
    if (!spk_shape_ok(N, T) || (size_t)N * T * s->cfg.n_mels >= ((size_t)1 << 31))
        return fail(GTTS_E_SHAPE, "gtts_spktrain_forward: %d sequences of %d frames exceed the 32-bit offsets", N, T);
    const SpkSaved sv = spk_saved(s, N, T);
    if (saved_bytes < sv.bytes) return fail(GTTS_E_WORKSPACE, "gtts_spktrain_forward: saved-state buffer too small");
    hipStream_t st = (hipStream_t)stream;
    const unsigned char *blob = static_cast<const unsigned char *>(packed);
    unsigned char *sb = static_cast<unsigned char *>(saved);
    const int H = s->cfg.hidden, E = s->cfg.embed, L = s->cfg.layers, M = N * T;
    float *hlast = (float *)(sb + sv.hlast);
    for (int l = 0; l < L; ++l) {
        SpkProjArgs pa;
        pa.wih = (const float4 *)(blob + s->off_wih[l]); pa.bias = (const float *)(blob + s->off_bias[l]);
        pa.x = l == 0 ? frames : (const float *)(sb + sv.Hs[l - 1]); pa.G = (float *)(sb + sv.A[l]);
        pa.M = M; pa.T = T; pa.K = l == 0 ? s->cfg.n_mels : H; pa.KB = s->kb[l];
        pa.sliced = 0; pa.P = 1; pa.S = 0; pa.T_total = T;
        GTTS_HIPCHK(spk_launch_proj(pa, st));
        SpkRecArgs ra;
        ra.whh = (const float4 *)(blob + s->off_whh[l]); ra.G = pa.G; ra.C = (float *)(sb + sv.C[l]);
        ra.hseq = (float *)(sb + sv.Hs[l]); ra.hlast = l + 1 == L ? hlast : nullptr;
        ra.N = N; ra.T = T;
        GTTS_HIPCHK(spk_launch_rec(ra, true, st));
    }
    GTTS_HIPCHK(spk_launch_head(hlast, (const float *)(blob + s->off_lin_wt), (const float *)(blob + s->off_lin_b), embeds, (float *)(sb + sv.raw),
                                N, H, E, st));
    return GTTS_OK;
}

extern "C" int gtts_spktrain_backward(const gtts_spk *s, const void *packed_train, const float *frames, const float *d_embeds, void *saved,
                                 size_t saved_bytes, float *const *grads, int n_grads, void *workspace, size_t workspace_bytes, int N, int T,
                                 gtts_stream_t stream) {
    if (!s || !packed_train || !frames || !d_embeds || !saved || !grads || !workspace) return fail(GTTS_E_NULL, "gtts_spktrain_backward: null argument");
    if (n_grads != (int)s->params.size()) return fail(GTTS_E_PARAMS, "spk: expected %d gradients, got %d", (int)s->params.size(), n_grads);
    for (int i = 0; i < n_grads; ++i)
        if (!grads[i]) return fail(GTTS_E_NULL, "spk: gradient of %s is null", s->params[i].name.c_str());
    if (N < 1 || T < 1) return fail(GTTS_E_SHAPE, "gtts_spktrain_backward: bad shape N=%d T=%d", N, T);
    if (!spk_shape_ok(N, T) || (size_t)N * T * s->cfg.n_mels >= ((size_t)1 << 31))
        return fail(GTTS_E_SHAPE, "gtts_spktrain_backward: %d sequences of %d frames exceed the 32-bit offsets", N, T);
    const SpkSaved sv = spk_saved(s, N, T);
    if (saved_bytes < sv.bytes) return fail(GTTS_E_WORKSPACE, "gtts_spktrain_backward: saved-state buffer too small");
    const SpkTrainWs wv = spk_train_ws(s, N, T);
    if (workspace_bytes < wv.bytes) return fail(GTTS_E_WORKSPACE, "gtts_spktrain_backward: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const unsigned char *blob = static_cast<const unsigned char *>(packed_train);
    unsigned char *sb = static_cast<unsigned char *>(saved), *ws = static_cast<unsigned char *>(workspace);
    const SpkTrainBlob tb = spk_train_blob(s);
    const int H = s->cfg.hidden, E = s->cfg.embed, L = s->cfg.layers, M = N * T;
    int SL, nsl;
    spk_slices(M, &SL, &nsl);
    float *dH = (float *)(ws + wv.dH), *dpre = (float *)(ws + wv.dpre), *dhlast = (float *)(ws + wv.dhlast);
    float *part = (float *)(ws + wv.part), *dbpart = (float *)(ws + wv.dbpart);
    const float *hlast = (const float *)(sb + sv.hlast);
    // head
    hipLaunchKernelGGL(spk_head_bwd_kernel, dim3((unsigned)N), dim3(256), (size_t)E * 4, st, (const float *)(sb + sv.raw), d_embeds,
                       (const float *)(blob + tb.lin_w), dpre, dhlast, H, E);
    GTTS_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(spk_lin_wgrad_kernel, dim3((unsigned)E), dim3(256), 0, st, (const float *)dpre, hlast, grads[4 * L], grads[4 * L + 1], N, H, E);
    GTTS_HIPCHK(hipGetLastError());
    const size_t lds = (size_t)2 * SPK_TILE * SPK_ZS * 4;
    GTTS_HIPCHK(raise_dyn_lds<&spk_rec_bwd_kernel>(lds));
    for (int l = L - 1; l >= 0; --l) {
        float *A = (float *)(sb + sv.A[l]);
        SpkRecBwdArgs ra;
        ra.whhT = (const float4 *)(blob + tb.whhT[l]); ra.A = A; ra.C = (const float *)(sb + sv.C[l]);
        ra.dH = l + 1 == L ? nullptr : dH; ra.dhlast = dhlast; ra.N = N; ra.T = T;
        hipLaunchKernelGGL(spk_rec_bwd_kernel, dim3((unsigned)((N + SPK_TILE - 1) / SPK_TILE)), dim3(64 * SPK_WAVES), lds, st, ra);
        GTTS_HIPCHK(hipGetLastError());
        if (l > 0) {
            hipLaunchKernelGGL(spk_dx_kernel, dim3((unsigned)((M + 63) / 64), SPK_H / 128), dim3(256), 0, st, (const float4 *)(blob + tb.wihT[l]),
                               (const float *)A, dH, M);
            GTTS_HIPCHK(hipGetLastError());
        }
        SpkWgradArgs wa;
        wa.dZ = A; wa.X = l == 0 ? frames : (const float *)(sb + sv.Hs[l - 1]); wa.Hs = (const float *)(sb + sv.Hs[l]); wa.part = part;
        wa.M = M; wa.T = T; wa.K = l == 0 ? s->cfg.n_mels : H; wa.nxt = s->kb[l]; wa.SL = SL;
        const int nct = wa.nxt + SPK_H / 16, NC = nct * 16;
        hipLaunchKernelGGL(spk_wgrad_kernel, dim3((unsigned)((nct + 7) / 8), SPK_G / 128, (unsigned)nsl), dim3(256), 0, st, wa);
        GTTS_HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(spk_colsum_kernel, dim3(SPK_G / 256, (unsigned)nsl), dim3(256), 0, st, (const float *)A, dbpart, M, SL);
        GTTS_HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(spk_wgrad_reduce_kernel, dim3((unsigned)((SPK_G * NC + 255) / 256)), dim3(256), 0, st, (const float *)part,
                           (const float *)dbpart, grads[4 * l], grads[4 * l + 1], grads[4 * l + 2], grads[4 * l + 3], wa.K, wa.nxt, nsl);
        GTTS_HIPCHK(hipGetLastError());
        if (wa.K == wa.nxt * 16) {                        // no padding column of X: the bias gradient has its own launch
            hipLaunchKernelGGL(spk_bias_reduce_kernel, dim3(SPK_G / 256), dim3(256), 0, st, (const float *)dbpart, grads[4 * l + 2], grads[4 * l + 3], nsl);
            GTTS_HIPCHK(hipGetLastError());
        }
    }
    return GTTS_OK;
}

// ---- GE2E
static bool ge2e_shape_ok(int S, int U, int E) {
    return S >= 1 && U >= 1 && E >= 1 && S <= GE2E_SMAX && (size_t)S * U * (size_t)(E > S ? E : S) < ((size_t)1 << 31);
}
static size_t ge2e_ws(int S, int U, int E, size_t off[9]) {
    const size_t R = (size_t)S * U;
    const size_t n[9] = {(size_t)S * E, (size_t)S * E, (size_t)S, R, R * S, 3 * R, (size_t)S * E, R * E, (size_t)S * E};
    size_t o = 0;
    for (int k = 0; k < 9; ++k) { off[k] = o; o += align256(n[k] * 4); }
    return o;
}
extern "C" size_t gtts_ge2e_workspace_bytes(int S, int U, int E) {
    size_t off[9];
    return ge2e_shape_ok(S, U, E) ? ge2e_ws(S, U, E, off) : 0;
}
extern "C" int gtts_ge2e_loss(const float *embeds, const float *w, const float *b, int S, int U, int E, float *sim, float *loss, float *d_embeds,
                              float *dw, float *db, void *workspace, size_t workspace_bytes, gtts_stream_t stream) {
    if (!embeds || !w || !b || !sim || !loss || !workspace) return fail(GTTS_E_NULL, "gtts_ge2e_loss: null argument");
    if (S < 1 || U < 1 || E < 1) return fail(GTTS_E_SHAPE, "gtts_ge2e_loss: bad shape S=%d U=%d E=%d", S, U, E);
    if (!ge2e_shape_ok(S, U, E))
        return fail(GTTS_E_SHAPE, "gtts_ge2e_loss: S=%d U=%d E=%d exceeds %d speakers or the 32-bit offsets", S, U, E, GE2E_SMAX);
    size_t off[9];
    if (workspace_bytes < ge2e_ws(S, U, E, off)) return fail(GTTS_E_WORKSPACE, "gtts_ge2e_loss: workspace too small");
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    Ge2eArgs a;
    a.emb = embeds; a.w = w; a.b = b; a.sim = sim; a.loss = loss; a.d_emb = d_embeds; a.dw = dw; a.db = db;
    float **wsp[9] = {&a.sum, &a.cin, &a.ynorm, &a.xnorm, &a.dcos, &a.rowpart, &a.dcin, &a.g, &a.dsum};
    for (int k = 0; k < 9; ++k) *wsp[k] = (float *)(ws + off[k]);
    a.S = S; a.U = U; a.E = E;
    hipLaunchKernelGGL(ge2e_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}
