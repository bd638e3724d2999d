// spk.hip -- DiffVC speaker encoder (DiffVC/speaker_encoder/encoder/model.py:43-63): a stack of torch.nn.LSTM(batch_first=True) layers
// with zero initial state, Linear + ReLU + L2 normalisation on the last layer's final hidden state, and (optionally) the mean and
// renormalisation of an utterance's partial embeddings (encoder/inference.py:150-151).  Gate order i, f, g, o; both biases.
// Per layer, two launches in stream order:
//   * spk_proj_kernel   G[n, t, :] = W_ih x[n, t] + (b_ih + b_hh) for all N * T rows at once -- the part of the gates that does not depend
//                       on the recurrence -- as a dense product on v_mfma_f32_16x16x4_f32 into the caller's workspace.  Layer 0 reads the
//                       rows of `frames` through the partial-utterance addressing (no stacked copy), layers above read the h sequence the
//                       layer below left in the workspace.
//   * spk_rec_kernel    one persistent workgroup per tile of SPK_TILE = 16 sequences walks all T steps: gates^T [4H x 16] =
//                       G^T + W_hh [4H x H] h_{t-1}^T [H x 16] on the same fp32 MFMA, then the cell update in registers.  W_hh (1 MB per
//                       layer) is streamed from L2 every step in MFMA fragment order (1 KB contiguous per wave-instruction, the next 16-wide
//                       k block in flight under the current one's 32 MFMAs, wrapping into the next step); h lives in LDS (double buffered,
//                       one workgroup barrier per step), c in registers.  No workgroup ever waits on another.
// Each wave owns 32 hidden units and computes their i, f, g, o rows, so the four gates of a (unit, sequence) pair meet in one lane's
// accumulators and the update needs no exchange.  An MFMA column is a sequence: a sequence's value is a fixed-order fp32 fmaf chain over
// its own data, whatever N is and whichever tile or column it lands in.  sigma and tanh are expf / tanhf (no fast-math forms).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gradtts_abi.h"
#include "common.h"
#include "kernels.h"
#include "spk.h"

namespace gtts {

// ---- weight packing: a [rows][K] row-major matrix -> MFMA A fragments.  Tile = 16 rows, k block = 16 columns; lane l of a fragment
// holds the four values W[row0 + (l & 15)][16 kb + 4 (l >> 4) + j], j = 0..3 -- the A operand of the block's four k steps (the k order
// inside a block is a fixed permutation, the same for the B operand).  dst[(tile * KB + kb) * 64 + lane]; columns >= K are zero.
// gate_order = 1 (W_hh): tile index = (unit group ug, gate g) -> rows g * H + 16 ug ..., so a wave's 8 tiles are contiguous.
__global__ void spk_pack_frag_kernel(const float *w, float4 *dst, int K, int KB, int ntiles, int gate_order) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ntiles * KB * 64) return;
    const int lane = idx & 63, kb = (idx >> 6) % KB, tile = (idx >> 6) / KB;
    const int row0 = gate_order ? (tile & 3) * SPK_H + (tile >> 2) * 16 : tile * 16;
    const float *src = w + (size_t)(row0 + (lane & 15)) * K;
    const int k = kb * 16 + (lane >> 4) * 4;
    float4 v;
    v.x = k < K ? src[k] : 0.f;
    v.y = k + 1 < K ? src[k + 1] : 0.f;
    v.z = k + 2 < K ? src[k + 2] : 0.f;
    v.w = k + 3 < K ? src[k + 3] : 0.f;
    dst[idx] = v;
}
// mode 0: dst[i] = a[i] + b[i] (the two gate biases);  mode 1: dst[k * rows + j] = a[j * cols + k] (Linear weight, transposed)
__global__ void spk_pack_misc_kernel(const float *a, const float *b, float *dst, int rows, int cols, int mode) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * cols) return;
    if (mode == 0) dst[idx] = a[idx] + b[idx];
    else dst[(size_t)(idx % cols) * rows + idx / cols] = a[idx];
}

// ---- input projection: G [M][4H] = X [M][K] W_ih^T + bias, M = N * T rows.  Workgroup: 4 waves, wave w = rows 16 (4 bx + w) ... of M
// against 8 row tiles (128 gate rows, blockIdx.y).  Computed transposed (A = W_ih fragment, B = X^T) so that a lane ends up with four
// consecutive gate rows of ONE row of M: a 16-byte store.
__global__ __launch_bounds__(256) void spk_proj_kernel(SpkProjArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sq = lane & 15, q = lane >> 4;
    const int m = (blockIdx.x * 4 + wave) * 16 + sq;
    const bool valid = m < a.M;
    const float *xrow = a.x;
    if (valid) {
        if (a.sliced) {
            const int n = m / a.T, t = m - n * a.T;
            xrow += ((size_t)(n / a.P) * a.T_total + (size_t)(n % a.P) * a.S + t) * a.K;
        } else {
            xrow += (size_t)m * a.K;
        }
    }
    const int rt0 = blockIdx.y * 8;
    f32x4 acc[8];
#pragma unroll
    for (int tl = 0; tl < 8; ++tl) acc[tl] = *reinterpret_cast<const f32x4 *>(a.bias + (rt0 + tl) * 16 + q * 4);
    const float4 *wp = a.wih + (size_t)rt0 * a.KB * 64 + lane;
    for (int kb = 0; kb < a.KB; ++kb) {
        const int k = kb * 16 + q * 4;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid && k < a.K) b = *reinterpret_cast<const float4 *>(xrow + k);         // K is a multiple of 4
        float4 w[8];
#pragma unroll
        for (int tl = 0; tl < 8; ++tl) w[tl] = wp[((size_t)tl * a.KB + kb) * 64];
#pragma unroll
        for (int tl = 0; tl < 8; ++tl) {
            acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[tl].x, b.x, acc[tl], 0, 0, 0);
            acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[tl].y, b.y, acc[tl], 0, 0, 0);
            acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[tl].z, b.z, acc[tl], 0, 0, 0);
            acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[tl].w, b.w, acc[tl], 0, 0, 0);
        }
    }
    if (valid) {
        float *g = a.G + (size_t)m * SPK_G + q * 4;
#pragma unroll
        for (int tl = 0; tl < 8; ++tl) *reinterpret_cast<f32x4 *>(g + (rt0 + tl) * 16) = acc[tl];
    }
}

// ---- the recurrence of one layer.  SAVE (training forward, spk_train.hip): the activated gates overwrite G and c_t goes to a.C;
// the arithmetic is the same, so both instances give the same bits.
template <bool SAVE>
__global__ __launch_bounds__(64 * SPK_WAVES) void spk_rec_kernel(SpkRecArgs a) {
    __shared__ __attribute__((aligned(16))) float hs[2][SPK_TILE][SPK_HS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sq = lane & 15, q = lane >> 4;
    const int n = blockIdx.x * SPK_TILE + sq;
    const bool valid = n < a.N;
    for (int i = tid; i < SPK_TILE * SPK_HS; i += 64 * SPK_WAVES) (&hs[0][0][0])[i] = 0.f;        // h_0 = 0
    float c[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) c[u][r] = 0.f;                                                  // c_0 = 0
    // this wave's 8 row tiles: tl = 4 * (unit group - 2 wave) + gate
    const float4 *wp = a.whh + (size_t)wave * 8 * SPK_KB * 64 + lane;
    float4 wcur[8], wnxt[8];
#pragma unroll
    for (int tl = 0; tl < 8; ++tl) wcur[tl] = wp[(tl * SPK_KB) * 64];
    const size_t row = (size_t)(valid ? n : 0) * a.T;
    lds_barrier();
#pragma unroll 1
    for (int t = 0; t < a.T; ++t) {
        const int p = t & 1;
        f32x4 acc[8];
        const float *g = a.G + (row + t) * SPK_G + q * 4;
#pragma unroll
        for (int tl = 0; tl < 8; ++tl) {
            const int r0 = (tl & 3) * SPK_H + (wave * 2 + (tl >> 2)) * 16;
            acc[tl] = valid ? *reinterpret_cast<const f32x4 *>(g + r0) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float *hb = &hs[p][sq][q * 4];
#pragma unroll 2
        for (int kb = 0; kb < SPK_KB; ++kb) {
            const int nk = (kb + 1) & (SPK_KB - 1);           // wraps: block 0 of the next step travels under the cell update
#pragma unroll
            for (int tl = 0; tl < 8; ++tl) wnxt[tl] = wp[(tl * SPK_KB + nk) * 64];
            const float4 b = *reinterpret_cast<const float4 *>(hb + kb * 16);
#pragma unroll
            for (int tl = 0; tl < 8; ++tl) acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(wcur[tl].x, b.x, acc[tl], 0, 0, 0);
#pragma unroll
            for (int tl = 0; tl < 8; ++tl) acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(wcur[tl].y, b.y, acc[tl], 0, 0, 0);
#pragma unroll
            for (int tl = 0; tl < 8; ++tl) acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(wcur[tl].z, b.z, acc[tl], 0, 0, 0);
#pragma unroll
            for (int tl = 0; tl < 8; ++tl) acc[tl] = __builtin_amdgcn_mfma_f32_16x16x4f32(wcur[tl].w, b.w, acc[tl], 0, 0, 0);
#pragma unroll
            for (int tl = 0; tl < 8; ++tl) wcur[tl] = wnxt[tl];
        }
        // cell update: lane = (sequence sq, units 16 ug + 4 q + r)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x4 h;
            [[maybe_unused]] f32x4 act[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float gi = sigmoid_f(acc[4 * u + 0][r]), gf = sigmoid_f(acc[4 * u + 1][r]);
                const float gg = tanhf(acc[4 * u + 2][r]), go = sigmoid_f(acc[4 * u + 3][r]);
                c[u][r] = fmaf(gf, c[u][r], gi * gg);
                h[r] = go * tanhf(c[u][r]);
                if constexpr (SAVE) { act[0][r] = gi; act[1][r] = gf; act[2][r] = gg; act[3][r] = go; }
            }
            const int unit = (wave * 2 + u) * 16 + q * 4;
            if constexpr (SAVE) {
                if (valid) {
                    float *ga = a.G + (row + t) * SPK_G + unit;
#pragma unroll
                    for (int k = 0; k < 4; ++k) *reinterpret_cast<f32x4 *>(ga + k * SPK_H) = act[k];
                    *reinterpret_cast<f32x4 *>(a.C + (row + t) * SPK_H + unit) = f32x4{c[u][0], c[u][1], c[u][2], c[u][3]};
                }
            }
            *reinterpret_cast<f32x4 *>(&hs[p ^ 1][sq][unit]) = h;
            if (valid) {
                if (a.hseq) *reinterpret_cast<f32x4 *>(a.hseq + (row + t) * SPK_H + unit) = h;
                if (a.hlast && t == a.T - 1) *reinterpret_cast<f32x4 *>(a.hlast + (size_t)n * SPK_H + unit) = h;
            }
        }
        lds_barrier();            // h_t complete before any wave reads it; every read of h_{t-1} was consumed before this point
    }
}

// ---- head: embeds[n] = relu(W h + b) / ||.||_2 (no epsilon: an all-zero row is 0 / 0 = NaN, as in the reference).  One workgroup per
// sequence; the reduction is a fixed tree.
__device__ __forceinline__ float spk_block_sum(float v, float *red) {
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

__global__ __launch_bounds__(256) void spk_head_kernel(const float *hlast, const float *wt, const float *bias, float *embeds, float *raw, int H, int E) {
    __shared__ float hsh[SPK_H];
    __shared__ float red[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    for (int k = tid; k < H; k += 256) hsh[k] = hlast[(size_t)n * H + k];
    __syncthreads();
    float *out = embeds + (size_t)n * E;
    float ss = 0.f;
    for (int j = tid; j < E; j += 256) {
        float acc = 0.f;
        for (int k = 0; k < H; ++k) acc = fmaf(wt[(size_t)k * E + j], hsh[k], acc);
        acc = fmaxf(acc + bias[j], 0.f);
        out[j] = acc;
        if (raw) raw[(size_t)n * E + j] = acc;                          // training: the un-normalised head output
        ss = fmaf(acc, acc, ss);
    }
    const float norm = sqrtf(spk_block_sum(ss, red));
    for (int j = tid; j < E; j += 256) out[j] = out[j] / norm;         // (each thread rereads its own stores)
}

// utt[u] = mean_p(embeds[u P + p]) / ||.||_2
__global__ __launch_bounds__(256) void spk_utt_kernel(const float *embeds, float *utt, int P, int E) {
    __shared__ float red[256];
    const int u = blockIdx.x, tid = threadIdx.x;
    float *out = utt + (size_t)u * E;
    float ss = 0.f;
    for (int j = tid; j < E; j += 256) {
        float s = 0.f;
        for (int p = 0; p < P; ++p) s += embeds[((size_t)u * P + p) * E + j];
        s = s / (float)P;
        out[j] = s;
        ss = fmaf(s, s, ss);
    }
    const float norm = sqrtf(spk_block_sum(ss, red));
    for (int j = tid; j < E; j += 256) out[j] = out[j] / norm;
}

// launchers shared with the training entry points (spk_train.hip)
hipError_t spk_launch_proj(const SpkProjArgs &pa, hipStream_t st) {
    hipLaunchKernelGGL(spk_proj_kernel, dim3((unsigned)((pa.M + 63) / 64), SPK_G / 128), dim3(256), 0, st, pa);
    return hipGetLastError();
}
hipError_t spk_launch_rec(const SpkRecArgs &ra, bool save, hipStream_t st) {
    const dim3 grid((unsigned)((ra.N + SPK_TILE - 1) / SPK_TILE)), block(64 * SPK_WAVES);
    if (save) hipLaunchKernelGGL(spk_rec_kernel<true>, grid, block, 0, st, ra);
    else hipLaunchKernelGGL(spk_rec_kernel<false>, grid, block, 0, st, ra);
    return hipGetLastError();
}
hipError_t spk_launch_head(const float *hlast, const float *wt, const float *bias, float *embeds, float *raw, int N, int H, int E, hipStream_t st) {
    hipLaunchKernelGGL(spk_head_kernel, dim3((unsigned)N), dim3(256), 0, st, hlast, wt, bias, embeds, raw, H, E);
    return hipGetLastError();
}

}  // namespace gtts

using namespace gtts;

extern "C" int gtts_spk_create(const gtts_spk_cfg *cfg, gtts_spk **out) {
    if (!cfg || !out) return fail(GTTS_E_NULL, "gtts_spk_create: null argument");
    const gtts_spk_cfg c = *cfg;
    if (c.hidden != SPK_H) return fail(GTTS_E_CONFIG, "spk: hidden must be %d (got %d)", SPK_H, c.hidden);
    if (c.n_mels < 4 || c.n_mels > 1024 || c.n_mels % 4 != 0)
        return fail(GTTS_E_CONFIG, "spk: n_mels must be a multiple of 4 in [4, 1024] (got %d)", c.n_mels);
    if (c.layers < 1 || c.layers > 8) return fail(GTTS_E_CONFIG, "spk: layers must lie in [1, 8] (got %d)", c.layers);
    if (c.embed < 1 || c.embed > 4096) return fail(GTTS_E_CONFIG, "spk: embed must lie in [1, 4096] (got %d)", c.embed);
    gtts_spk *s = new gtts_spk();
    s->cfg = c;
    size_t o = 0;
    for (int l = 0; l < c.layers; ++l) {
        const int K = l == 0 ? c.n_mels : c.hidden;
        const std::string sfx = "_l" + std::to_string(l);
        s->params.push_back({"lstm.weight_ih" + sfx, 2, {SPK_G, K, 0, 0}});
        s->params.push_back({"lstm.weight_hh" + sfx, 2, {SPK_G, c.hidden, 0, 0}});
        s->params.push_back({"lstm.bias_ih" + sfx, 1, {SPK_G, 0, 0, 0}});
        s->params.push_back({"lstm.bias_hh" + sfx, 1, {SPK_G, 0, 0, 0}});
        s->kb.push_back((K + 15) / 16);
        s->off_wih.push_back(o); o += align256((size_t)(SPK_G / 16) * s->kb[l] * 64 * 16);
        s->off_whh.push_back(o); o += align256((size_t)(SPK_G / 16) * SPK_KB * 64 * 16);
        s->off_bias.push_back(o); o += align256((size_t)SPK_G * 4);
    }
    s->params.push_back({"linear.weight", 2, {c.embed, c.hidden, 0, 0}});
    s->params.push_back({"linear.bias", 1, {c.embed, 0, 0, 0}});
    s->off_lin_wt = o; o += align256((size_t)c.embed * c.hidden * 4);
    s->off_lin_b = o; o += align256((size_t)c.embed * 4);
    s->blob_bytes = o;
    *out = s;
    return GTTS_OK;
}

extern "C" void gtts_spk_destroy(gtts_spk *s) { delete s; }

extern "C" int gtts_spk_num_params(const gtts_spk *s) { return s ? (int)s->params.size() : fail(GTTS_E_NULL, "gtts_spk_num_params: null handle"); }

extern "C" int gtts_spk_param_info(const gtts_spk *s, int i, const char **name, int *rank, int dims[4]) {
    if (!s) return fail(GTTS_E_NULL, "gtts_spk_param_info: null handle");
    if (i < 0 || i >= (int)s->params.size()) return fail(GTTS_E_PARAMS, "gtts_spk_param_info: index %d out of range", i);
    if (name) *name = s->params[i].name.c_str();
    if (rank) *rank = s->params[i].rank;
    if (dims) for (int k = 0; k < 4; ++k) dims[k] = s->params[i].dims[k];
    return GTTS_OK;
}

extern "C" size_t gtts_spk_packed_bytes(const gtts_spk *s) { return s ? s->blob_bytes : 0; }

extern "C" int gtts_spk_pack(const gtts_spk *s, const void *const *ptrs, int n, void *packed, gtts_stream_t stream) {
    if (!s || !ptrs || !packed) return fail(GTTS_E_NULL, "gtts_spk_pack: null argument");
    if (n != (int)s->params.size()) return fail(GTTS_E_PARAMS, "spk: expected %d parameters, got %d", (int)s->params.size(), n);
    for (int i = 0; i < n; ++i)
        if (!ptrs[i]) return fail(GTTS_E_NULL, "spk: parameter %s is null", s->params[i].name.c_str());
    hipStream_t st = (hipStream_t)stream;
    unsigned char *blob = static_cast<unsigned char *>(packed);
    const int H = s->cfg.hidden, E = s->cfg.embed;
    for (int l = 0; l < s->cfg.layers; ++l) {
        const int K = l == 0 ? s->cfg.n_mels : H;
        const float *wih = (const float *)ptrs[4 * l], *whh = (const float *)ptrs[4 * l + 1];
        const float *bih = (const float *)ptrs[4 * l + 2], *bhh = (const float *)ptrs[4 * l + 3];
        int cnt = (SPK_G / 16) * s->kb[l] * 64;
        hipLaunchKernelGGL(spk_pack_frag_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, wih, (float4 *)(blob + s->off_wih[l]), K, s->kb[l],
                           SPK_G / 16, 0);
        GTTS_HIPCHK(hipGetLastError());
        cnt = (SPK_G / 16) * SPK_KB * 64;
        hipLaunchKernelGGL(spk_pack_frag_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, whh, (float4 *)(blob + s->off_whh[l]), H, SPK_KB,
                           SPK_G / 16, 1);
        GTTS_HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(spk_pack_misc_kernel, dim3((SPK_G + 255) / 256), dim3(256), 0, st, bih, bhh, (float *)(blob + s->off_bias[l]), SPK_G, 1, 0);
        GTTS_HIPCHK(hipGetLastError());
    }
    const float *lw = (const float *)ptrs[4 * s->cfg.layers], *lb = (const float *)ptrs[4 * s->cfg.layers + 1];
    hipLaunchKernelGGL(spk_pack_misc_kernel, dim3((E * H + 255) / 256), dim3(256), 0, st, lw, (const float *)nullptr,
                       (float *)(blob + s->off_lin_wt), E, H, 1);
    GTTS_HIPCHK(hipGetLastError());
    GTTS_HIPCHK(hipMemcpyAsync(blob + s->off_lin_b, lb, (size_t)E * 4, hipMemcpyDeviceToDevice, st));
    return GTTS_OK;
}

// workspace: G [N T][4H], hseq [N T][H] (layers below the last), hlast [N][H]
bool gtts::spk_shape_ok(int N, int T) { return N >= 1 && T >= 1 && (size_t)N * (size_t)T * SPK_G < ((size_t)1 << 31); }
static size_t spk_ws(const gtts_spk *s, int N, int T, size_t off[3]) {
    const size_t rows = (size_t)N * T;
    off[0] = 0;
    off[1] = align256(rows * SPK_G * 4);
    off[2] = off[1] + (s->cfg.layers > 1 ? align256(rows * SPK_H * 4) : 0);
    return off[2] + align256((size_t)N * SPK_H * 4);
}

extern "C" size_t gtts_spk_workspace_bytes(const gtts_spk *s, int N, int T) {
    if (!s || !spk_shape_ok(N, T)) return 0;
    size_t off[3];
    return spk_ws(s, N, T, off);
}

extern "C" int gtts_spk_forward(const gtts_spk *s, const void *packed, const float *frames, int U, int T_total, int P, int S, int T,
                                float *embeds, float *hidden_out, float *utt_embeds, void *workspace, size_t workspace_bytes,
                                gtts_stream_t stream) {
    if (!s || !packed || !frames || !embeds || !workspace) return fail(GTTS_E_NULL, "gtts_spk_forward: null argument");
    if (U < 1 || P < 1 || T < 1 || T_total < 1 || S < 0)
        return fail(GTTS_E_SHAPE, "gtts_spk_forward: bad shape U=%d T_total=%d P=%d S=%d T=%d", U, T_total, P, S, T);
    if ((long long)(P - 1) * S + T > (long long)T_total)
        return fail(GTTS_E_SHAPE, "gtts_spk_forward: partial %d of %d frames at step %d ends beyond the %d frames of an utterance", P - 1, T, S, T_total);
    if ((long long)U * P > 0x7fffffff / SPK_G || !spk_shape_ok(U * P, T) || (size_t)U * T_total * s->cfg.n_mels >= ((size_t)1 << 31))
        return fail(GTTS_E_SHAPE, "gtts_spk_forward: %d x %d sequences of %d frames exceed the 32-bit offsets", U, P, T);
    const int N = U * P, H = s->cfg.hidden, E = s->cfg.embed, L = s->cfg.layers;
    size_t off[3];
    if (workspace_bytes < spk_ws(s, N, T, off)) return fail(GTTS_E_WORKSPACE, "gtts_spk_forward: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const unsigned char *blob = static_cast<const unsigned char *>(packed);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    float *G = (float *)(ws + off[0]), *hseq = (float *)(ws + off[1]);
    float *hlast = hidden_out ? hidden_out : (float *)(ws + off[2]);
    const int M = N * T;
    for (int l = 0; l < L; ++l) {
        SpkProjArgs pa;
        pa.wih = (const float4 *)(blob + s->off_wih[l]); pa.bias = (const float *)(blob + s->off_bias[l]);
        pa.x = l == 0 ? frames : hseq; pa.G = G;
        pa.M = M; pa.T = T; pa.K = l == 0 ? s->cfg.n_mels : H; pa.KB = s->kb[l];
        pa.sliced = l == 0; pa.P = P; pa.S = S; pa.T_total = T_total;
        GTTS_HIPCHK(spk_launch_proj(pa, st));
        SpkRecArgs ra;
        ra.whh = (const float4 *)(blob + s->off_whh[l]); ra.G = G; ra.C = nullptr;
        ra.hseq = l + 1 < L ? hseq : nullptr; ra.hlast = l + 1 == L ? hlast : nullptr;
        ra.N = N; ra.T = T;
        GTTS_HIPCHK(spk_launch_rec(ra, false, st));
    }
    GTTS_HIPCHK(spk_launch_head(hlast, (const float *)(blob + s->off_lin_wt), (const float *)(blob + s->off_lin_b), embeds, nullptr, N, H, E, st));
    if (utt_embeds) {
        hipLaunchKernelGGL(spk_utt_kernel, dim3((unsigned)U), dim3(256), 0, st, (const float *)embeds, utt_embeds, P, E);
        GTTS_HIPCHK(hipGetLastError());
    }
    return GTTS_OK;
}
