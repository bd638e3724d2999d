// misc.hip -- the bandwidth-bound and tiny kernels around the MFMA convolutions (gfx950).
//   prep_input      torch.stack([mu, x(, s)], 1)                       diffusion.py:181-185
//   spk_mlp         spk_mlp(spk)                                       diffusion.py:139-141,176
//   time_mlp        SinusoidalPosEmb -> mlp -> per-ResnetBlock Linear(Mish(t))   diffusion.py:118-125,143-144,64-65,76
//   gn_finalize     GroupNorm statistics -> per-(sample, channel) scale/shift    diffusion.py:53 (eps 1e-5, biased var)
//   tail_identity   ResnetBlock tail with Identity res_conv: Mish(GN(h))*mask + x*mask   diffusion.py:58,72,78
//   final_euler     final_block GN/Mish/mask + final_conv 1x1 + mask (+ Euler update)    diffusion.py:213-216,264-274
//   euler_step      one reverse-diffusion update                                          diffusion.py:264-274
#include "common.h"
#include "kernels.h"

namespace gtts {

// ------------------------------------------------------------------------------------------------ prep_input
template <typename AT>
__global__ void prep_input_kernel(const float *__restrict__ mu, const float *__restrict__ x,
                                  const float *__restrict__ s, AT *__restrict__ x0, int F, int T, int nch) {
    // grid: (ceil(F*T/256), nch, B)
    const int b = blockIdx.z, c = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F * T) return;
    float v;
    if (c == 0) v = mu[(size_t)b * F * T + i];
    else if (c == 1) v = x[(size_t)b * F * T + i];
    else v = s[(size_t)b * F + i / T];     // speaker channel: constant along frames (diffusion.py:184)
    x0[((size_t)b * nch + c) * F * T + i] = (AT)v;
}

template <typename AT>
static hipError_t launch_prep_input_t(const float *mu, const float *x, const float *s, void *x0, int B, int F, int T, int nch,
                                      hipStream_t st, std::string *name) {
    if (name) return kernel_name(name, "gtts::prep_input_kernel", act_name<AT>());
    hipLaunchKernelGGL(prep_input_kernel<AT>, dim3((F * T + 255) / 256, nch, B), dim3(256), 0, st, mu, x, s, (AT *)x0, F, T, nch);
    return hipGetLastError();
}
hipError_t launch_prep_input(const float *mu, const float *x, const float *s, void *x0, int B, int F, int T,
                             int nch, hipStream_t st, int act_bf16, std::string *name) {
    return act_bf16 ? launch_prep_input_t<__bf16>(mu, x, s, x0, B, F, T, nch, st, name)
                    : launch_prep_input_t<float>(mu, x, s, x0, B, F, T, nch, st, name);
}

// ------------------------------------------------------------------------------------------------ small MLPs
__device__ __forceinline__ float dot_row(const float *__restrict__ w, const float *v, int n) {
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc = fmaf(w[i], v[i], acc);
    return acc;
}

// spk_mlp: Linear(E -> 4E) -> Mish -> Linear(4E -> F);   one workgroup per sample
__global__ void spk_mlp_kernel(const float *__restrict__ spk, const float *__restrict__ w0,
                               const float *__restrict__ b0, const float *__restrict__ w2,
                               const float *__restrict__ b2, float *__restrict__ s, int E, int F) {
    extern __shared__ float sm[];
    float *e = sm, *h = sm + E;
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < E; i += blockDim.x) e[i] = spk[(size_t)b * E + i];
    __syncthreads();
    for (int j = threadIdx.x; j < 4 * E; j += blockDim.x) h[j] = mish_f(b0[j] + dot_row(w0 + (size_t)j * E, e, E));
    __syncthreads();
    for (int j = threadIdx.x; j < F; j += blockDim.x) s[(size_t)b * F + j] = b2[j] + dot_row(w2 + (size_t)j * 4 * E, h, 4 * E);
}

hipError_t launch_spk_mlp(const float *spk, const float *w0, const float *b0, const float *w2, const float *b2,
                          float *s, int B, int E, int F, hipStream_t st) {
    hipLaunchKernelGGL(spk_mlp_kernel, dim3(B), dim3(256), (size_t)5 * E * sizeof(float), st, spk, w0, b0, w2, b2, s,
                       E, F);
    return hipGetLastError();
}

// time_mlp: one workgroup per (step, sample) row.  freq[] is computed on the host exactly as the reference does
// (torch.exp(arange(half).float() * -log(1e4)/(half-1)) on CPU), so the sin/cos arguments are bit-identical.
__global__ void time_mlp_kernel(const float *__restrict__ t, const float *__restrict__ freq, float pe_scale,
                                const unsigned char *__restrict__ blob, TimeMlpDesc d, float *__restrict__ tb) {
    extern __shared__ float sm[];
    const int dim = d.dim, half = dim / 2;
    float *emb = sm, *h = sm + dim, *t2 = h + 4 * dim;
    const int row = blockIdx.x;
    const float tv = t[row];
    for (int k = threadIdx.x; k < half; k += blockDim.x) {
        const float arg = __fmul_rn(__fmul_rn(pe_scale, tv), freq[k]);   // scale * x * emb  (diffusion.py:123)
        const float sv = sinf(arg), cv = cosf(arg);
        emb[k] = sv;
        emb[half + k] = cv;
        if (d.semb_off >= 0) {                                            // DiffVC: `condition` starts with it
            tb[(size_t)row * d.tb_stride + d.semb_off + k] = sv;
            tb[(size_t)row * d.tb_stride + d.semb_off + half + k] = cv;
        }
    }
    __syncthreads();
    const float *w0 = reinterpret_cast<const float *>(blob + d.w0), *b0 = reinterpret_cast<const float *>(blob + d.b0);
    const float *w2 = reinterpret_cast<const float *>(blob + d.w2), *b2 = reinterpret_cast<const float *>(blob + d.b2);
    for (int j = threadIdx.x; j < 4 * dim; j += blockDim.x) h[j] = mish_f(b0[j] + dot_row(w0 + (size_t)j * dim, emb, dim));
    __syncthreads();
    for (int j = threadIdx.x; j < dim; j += blockDim.x) {
        const float v = b2[j] + dot_row(w2 + (size_t)j * 4 * dim, h, 4 * dim);
        t2[j] = v;
        tb[(size_t)row * d.tb_stride + d.temb_off + j] = v;    // raw time embedding (DiffVC RefBlock / tests)
    }
    __syncthreads();
    for (int j = threadIdx.x; j < dim; j += blockDim.x) emb[j] = mish_f(t2[j]);   // Mish() of ResnetBlock.mlp
    __syncthreads();
    for (int r = 0; r < d.n; ++r) {
        const float *w = reinterpret_cast<const float *>(blob + d.w[r]);
        const float *bb = reinterpret_cast<const float *>(blob + d.b[r]);
        for (int co = threadIdx.x; co < d.cout[r]; co += blockDim.x)
            tb[(size_t)row * d.tb_stride + d.off[r] + co] = bb[co] + dot_row(w + (size_t)co * dim, emb, dim);
    }
}

hipError_t launch_time_mlp(const float *t, const float *freq, float pe_scale, const unsigned char *blob,
                           const TimeMlpDesc &d, float *tb, int rows, hipStream_t st) {
    hipLaunchKernelGGL(time_mlp_kernel, dim3(rows), dim3(256), (size_t)6 * d.dim * sizeof(float), st, t, freq,
                       pe_scale, blob, d, tb);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ gn_finalize
// partials [B][nparts][groups][2] (fp32 sums of x and x^2 per workgroup tile, fixed order) ->
// scale[b][c] = gamma[c] * rstd,  shift[b][c] = beta[c] - mean * scale.   One workgroup per sample, one wave per
// group, double accumulation, fixed reduction order => bit-reproducible run to run.  The kernel is pure latency:
// the partial loads are issued four deep before the dependent fp64 adds.
__global__ void gn_finalize_kernel(const float *__restrict__ partials, int nparts, int groups, int C, float count,
                                   const float *__restrict__ gamma, const float *__restrict__ beta,
                                   float *__restrict__ sc, float *__restrict__ sh) {
    const int b = blockIdx.x;
    const int g = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (g >= groups) return;
    double s1 = 0.0, s2 = 0.0;
    const float2 *p = reinterpret_cast<const float2 *>(partials) + (size_t)b * nparts * groups + g;
    for (int i0 = l; i0 < nparts; i0 += 256) {
        float2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + 64 * u;
            v[u] = i < nparts ? p[(size_t)i * groups] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s1 += (double)v[u].x;
            s2 += (double)v[u].y;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
    }
    const double mean = s1 / (double)count;
    double var = s2 / (double)count - mean * mean;
    if (var < 0.0) var = 0.0;
    const double rstd = 1.0 / sqrt(var + 1e-5);
    const int gs = C / groups;
    for (int c = g * gs + l; c < (g + 1) * gs; c += 64) {
        const double a = (double)gamma[c] * rstd;
        sc[(size_t)b * C + c] = (float)a;
        sh[(size_t)b * C + c] = (float)((double)beta[c] - mean * a);
    }
}

hipError_t launch_gn_finalize(const float *partials, int nparts, int groups, int C, int HW, const float *gamma,
                              const float *beta, float *sc, float *sh, int B, hipStream_t st) {
    if (groups * 64 > 1024) return hipErrorInvalidValue;
    const float count = (float)((double)(C / groups) * (double)HW);
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(B), dim3(groups * 64), 0, st, partials, nparts, groups, C, count,
                       gamma, beta, sc, sh);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ tail_identity
// 4 consecutive activations as fp32, from fp32 or bf16 storage
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 ld4(const __bf16 *p) {
    const uint2 u = *reinterpret_cast<const uint2 *>(p);
    return make_float4(__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                       __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u));
}
__device__ __forceinline__ void st4(float *p, float4 v) {
    typedef __attribute__((ext_vector_type(4))) float f32x4s;
    if (GTTS_OUT_NT) {
        f32x4s q;
        q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
        __builtin_nontemporal_store(q, reinterpret_cast<f32x4s *>(p));
    } else *reinterpret_cast<float4 *>(p) = v;
}
__device__ __forceinline__ void st4(__bf16 *p, float4 v) {
    typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
    bf16x4 o;
    o[0] = (__bf16)v.x; o[1] = (__bf16)v.y; o[2] = (__bf16)v.z; o[3] = (__bf16)v.w;
    *reinterpret_cast<bf16x4 *>(p) = o;
}

// ITEMS (VEC-wide) items per thread, one block-stride apart; all loads of a thread are issued before the first use.
// Measured (round 4): neither 16-byte bf16 accesses nor four items per thread (a quarter of the workgroups) move this kernel --
// 64-72 us per launch in fp32 AND in bf16 storage (5.3 vs 2.9 TB/s): at two transcendentals + ~12 VALU per element Mish itself
// is ~45 us of issue time at level 0, so the bf16 form is VALU-bound, the fp32 form HBM-bound, at about the same time.
template <int VEC, typename AT, int ITEMS>
__global__ __launch_bounds__(256) void tail_identity_kernel(const AT *__restrict__ h, const AT *__restrict__ x,
                                     const float *__restrict__ sc, const float *__restrict__ sh,
                                     const float *__restrict__ mask, AT *__restrict__ out, int C, int H, int W,
                                     int T, int lvl) {
    // grid: (ceil(H*W/VEC/256/ITEMS), C, B): one (sample, channel) plane per blockIdx.(y,z) -> scalar scale/shift
    const int b = blockIdx.z, c = blockIdx.y;
    const int HW = H * W;
    const int i0 = (blockIdx.x * ITEMS * 256 + threadIdx.x) * VEC;
    if (i0 >= HW) return;
    const float a = sc[(size_t)b * C + c], s = sh[(size_t)b * C + c];
    const size_t plane = ((size_t)b * C + c) * HW;
    const float *mp = mask + (size_t)b * T;
    if constexpr (VEC == 8) {
        // bf16 storage, 16-byte accesses (8 activations per lane)
        static_assert(VEC != 8 || sizeof(AT) == 2, "VEC 8 is the bf16-storage form");
        u32x4 hu[ITEMS], xu[ITEMS];
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const int i = min(i0 + it * 256 * VEC, HW - VEC);          // (clamped: the extra loads are never used)
            hu[it] = *reinterpret_cast<const u32x4 *>(h + plane + i);
            xu[it] = *reinterpret_cast<const u32x4 *>(x + plane + i);
        }
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const int i = i0 + it * 256 * VEC;
            if (i >= HW) break;
            const int col = i % W;
            u32x4 ou;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float m0 = mp[(size_t)(col + 2 * q) << lvl], m1 = mp[(size_t)(col + 2 * q + 1) << lvl];
                const float h0 = __builtin_bit_cast(float, hu[it][q] << 16), h1 = __builtin_bit_cast(float, hu[it][q] & 0xffff0000u);
                const float x0 = __builtin_bit_cast(float, xu[it][q] << 16), x1 = __builtin_bit_cast(float, xu[it][q] & 0xffff0000u);
                const __bf16 o0 = (__bf16)(mish_f(h0 * a + s) * m0 + x0 * m0), o1 = (__bf16)(mish_f(h1 * a + s) * m1 + x1 * m1);
                ou[q] = (unsigned)__builtin_bit_cast(unsigned short, o0) | ((unsigned)__builtin_bit_cast(unsigned short, o1) << 16);
            }
            *reinterpret_cast<u32x4 *>(out + plane + i) = ou;
        }
    } else if constexpr (VEC == 4) {
        float4 hv[ITEMS], xv[ITEMS];
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const int i = min(i0 + it * 256 * VEC, HW - VEC);
            hv[it] = ld4(h + plane + i);
            xv[it] = ld4(x + plane + i);
        }
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const int i = i0 + it * 256 * VEC;
            if (i >= HW) break;
            const int col = i % W;
            const float m0 = mp[(size_t)(col + 0) << lvl], m1 = mp[(size_t)(col + 1) << lvl];
            const float m2 = mp[(size_t)(col + 2) << lvl], m3 = mp[(size_t)(col + 3) << lvl];
            float4 o;
            o.x = tail_value(hv[it].x, xv[it].x, a, s, m0);
            o.y = tail_value(hv[it].y, xv[it].y, a, s, m1);
            o.z = tail_value(hv[it].z, xv[it].z, a, s, m2);
            o.w = tail_value(hv[it].w, xv[it].w, a, s, m3);
            st4(out + plane + i, o);
        }
    } else {
        static_assert(VEC != 1 || ITEMS == 1, "the scalar form takes one item per thread");
        const int col = i0 % W;
        const float m = mask[(size_t)b * T + ((size_t)col << lvl)];
        if constexpr (sizeof(AT) == 4) out[plane + i0] = (AT)tail_value((float)h[plane + i0], (float)x[plane + i0], a, s, m);
        else out[plane + i0] = (AT)(mish_f((float)h[plane + i0] * a + s) * m + (float)x[plane + i0] * m);
    }
}

template <int VEC, typename AT, int ITEMS>
static hipError_t launch_tail_items(const AT *h, const AT *x, const float *sc, const float *sh, const float *mask, AT *out, dim3 grid,
                                    int C, int H, int W, int T, int lvl, hipStream_t st, std::string *name) {
    if (name) return kernel_name(name, "gtts::tail_identity_kernel", VEC, act_name<AT>(), ITEMS);
    hipLaunchKernelGGL((tail_identity_kernel<VEC, AT, ITEMS>), grid, dim3(256), 0, st, h, x, sc, sh, mask, out, C, H, W, T, lvl);
    return hipGetLastError();
}
template <int VEC, typename AT>
static hipError_t launch_tail_vec(const AT *h, const AT *x, const float *sc, const float *sh, const float *mask, AT *out, int B, int C,
                                  int H, int W, int T, int lvl, hipStream_t st, std::string *name) {
    const int per_plane = (H * W / VEC + 255) / 256;        // one-item blocks per (sample, channel) plane
    if constexpr (VEC > 1) {      // (the scalar form takes one item per thread)
        if (per_plane >= 8)
            return launch_tail_items<VEC, AT, 4>(h, x, sc, sh, mask, out, dim3((per_plane + 3) / 4, C, B), C, H, W, T, lvl, st, name);
    }
    return launch_tail_items<VEC, AT, 1>(h, x, sc, sh, mask, out, dim3(per_plane, C, B), C, H, W, T, lvl, st, name);
}

template <typename AT>
static hipError_t launch_tail_identity_t(const AT *h, const AT *x, const float *sc, const float *sh, const float *mask,
                                         AT *out, int B, int C, int H, int W, int T, int lvl, hipStream_t st, std::string *name) {
    if constexpr (sizeof(AT) == 2) {
        if (W % 8 == 0) return launch_tail_vec<8, AT>(h, x, sc, sh, mask, out, B, C, H, W, T, lvl, st, name);
    }
    if (W % 4 == 0) return launch_tail_vec<4, AT>(h, x, sc, sh, mask, out, B, C, H, W, T, lvl, st, name);
    return launch_tail_vec<1, AT>(h, x, sc, sh, mask, out, B, C, H, W, T, lvl, st, name);
}
hipError_t launch_tail_identity(const void *h, const void *x, const float *sc, const float *sh, const float *mask,
                                void *out, int B, int C, int H, int W, int T, int lvl, hipStream_t st, int act_bf16, std::string *name) {
    if (act_bf16) return launch_tail_identity_t((const __bf16 *)h, (const __bf16 *)x, sc, sh, mask, (__bf16 *)out, B, C, H, W, T, lvl, st, name);
    return launch_tail_identity_t((const float *)h, (const float *)x, sc, sh, mask, (float *)out, B, C, H, W, T, lvl, st, name);
}

// ------------------------------------------------------------------------------------------------ Euler update
// Exactly the reference's fp32 operation order (diffusion.py:264-274); explicit *_rn intrinsics forbid FMA
// contraction so that, given the same estimator output, the update is bit-identical to the CPU path.
__device__ __forceinline__ float euler_update(float xt, float mu, float est, float m, float noise, bool stoc,
                                              float beta, float h, float sq) {
    float dxt;
    if (stoc) {
        float det = __fsub_rn(__fmul_rn(0.5f, __fsub_rn(mu, xt)), est);      // 0.5*(mu - xt) - est
        det = __fmul_rn(__fmul_rn(det, beta), h);                            // * noise_t * h
        dxt = __fadd_rn(det, __fmul_rn(noise, sq));                          // + randn * sqrt(noise_t*h)
    } else {
        dxt = __fmul_rn(0.5f, __fsub_rn(__fsub_rn(mu, xt), est));            // 0.5*(mu - xt - est)
        dxt = __fmul_rn(__fmul_rn(dxt, beta), h);
    }
    return __fmul_rn(__fsub_rn(xt, dxt), m);                                 // (xt - dxt) * mask
}

__global__ void euler_step_kernel(float *__restrict__ xt, const float *__restrict__ mu,
                                  const float *__restrict__ est, const float *__restrict__ mask,
                                  const float *__restrict__ noise, float beta, float h, float sq, int F, int T,
                                  size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int col = (int)(i % T);
    const size_t b = i / ((size_t)F * T);
    const float m = mask[b * T + col];
    xt[i] = euler_update(xt[i], mu[i], est[i], m, noise ? noise[i] : 0.f, noise != nullptr, beta, h, sq);
}

hipError_t launch_euler_step(float *xt, const float *mu, const float *est, const float *mask, const float *noise,
                             float beta, float h, int B, int F, int T, hipStream_t st) {
    const size_t total = (size_t)B * F * T;
    const float sq = sqrtf(beta * h);     // torch.sqrt(noise_t * h) in fp32
    hipLaunchKernelGGL(euler_step_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, xt, mu, est, mask,
                       noise, beta, h, sq, F, T, total);
    return hipGetLastError();
}

__global__ void mul_mask_kernel(const float *__restrict__ z, const float *__restrict__ mask, float *__restrict__ out,
                                int F, int T, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int col = (int)(i % T);
    const size_t b = i / ((size_t)F * T);
    out[i] = __fmul_rn(z[i], mask[b * T + col]);
}

hipError_t launch_mul_mask(const float *z, const float *mask, float *out, int B, int F, int T, hipStream_t st) {
    const size_t total = (size_t)B * F * T;
    hipLaunchKernelGGL(mul_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, z, mask, out, F, T,
                       total);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ final_euler
// est = (sum_c w[c] * (Mish(GN(raw[c])) * m) * m + bias) * m        (final_block :56-58, final_conv :214-216)
// then optionally the Euler update of xt in the same pass (est never touches HBM inside the sampling loop).
// DiffVC update (DiffVC/model/diffusion.py:177-195), same fp32 operation order as the reference's tensor math:
//   pf:     dxt = 0.5*(mean - xt - est) * (beta*h)
//   em/ml:  dxt = (mean - xt)*cm;  dxt -= est*k1*bh;  dxt += randn*sigma          xt = (xt - dxt)*mask
__device__ __forceinline__ float vc_update(float xt, float mean, float est, float m, float noise, int mode, float cm,
                                           float k1, float bh, float sigma) {
    float dxt;
    if (mode == 1) {
        dxt = __fmul_rn(__fmul_rn(0.5f, __fsub_rn(__fsub_rn(mean, xt), est)), bh);
    } else {
        dxt = __fmul_rn(__fsub_rn(mean, xt), cm);
        dxt = __fsub_rn(dxt, __fmul_rn(__fmul_rn(est, k1), bh));
        dxt = __fadd_rn(dxt, __fmul_rn(noise, sigma));
    }
    return __fmul_rn(__fsub_rn(xt, dxt), m);
}

// PX consecutive frames per thread (T % PX == 0): bf16 storage takes PX = 4 (8-byte loads; 2-byte accesses ran at 2.9 TB/s)
template <typename AT, int PX>
__global__ void final_euler_kernel(const AT *__restrict__ raw, const float *__restrict__ sc,
                                   const float *__restrict__ sh, const float *__restrict__ w, const float *__restrict__ bias,
                                   const float *__restrict__ mask, int C, int F, int T, float *__restrict__ est_out,
                                   float *__restrict__ xt, const float *__restrict__ mu, const float *__restrict__ noise,
                                   float beta, float h, float sq, VcStep vc) {
    extern __shared__ float sm[];     // [3][C]: scale, shift, weight
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < C; i += 256) {
        sm[i] = sc[(size_t)b * C + i];
        sm[C + i] = sh[(size_t)b * C + i];
        sm[2 * C + i] = w[i];
    }
    __syncthreads();
    const int i = (blockIdx.x * 256 + threadIdx.x) * PX;
    const int FT = F * T;
    if (i >= FT) return;
    const int col = i % T;
    float m[PX], acc[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) { m[j] = mask[(size_t)b * T + col + j]; acc[j] = 0.f; }
    const AT *p = raw + (size_t)b * C * FT + i;
    for (int c = 0; c < C; ++c) {
        float r[PX];
        if constexpr (PX == 4 && sizeof(AT) == 2) {
            const float4 v4 = ld4(p + (size_t)c * FT);
            r[0] = v4.x; r[1] = v4.y; r[2] = v4.z; r[3] = v4.w;
        } else {
#pragma unroll
            for (int j = 0; j < PX; ++j) r[j] = (float)p[(size_t)c * FT + j];
        }
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const float v = mish_f(r[j] * sm[c] + sm[C + c]) * m[j] * m[j];
            acc[j] = fmaf(sm[2 * C + c], v, acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        const float est = (acc[j] + bias[0]) * m[j];
        const size_t o = (size_t)b * FT + i + j;
        if (est_out) est_out[o] = est;
        if (xt) {
            if (vc.mode == 0) xt[o] = euler_update(xt[o], mu[o], est, m[j], noise ? noise[o] : 0.f, noise != nullptr, beta, h, sq);
            else xt[o] = vc_update(xt[o], mu[o], est, m[j], noise ? noise[o] : 0.f, vc.mode, vc.cm, vc.k1, vc.bh, vc.sigma);
        }
    }
}

template <typename AT, int VEC>
static hipError_t launch_final_euler_t(const void *raw, const float *sc, const float *sh, const float *w, const float *bias,
                                       const float *mask, int B, int C, int F, int T, float *est_out, float *xt, const float *mu,
                                       const float *noise, float beta, float h, hipStream_t st, const VcStep &v, std::string *name) {
    if (name) return kernel_name(name, "gtts::final_euler_kernel", act_name<AT>(), VEC);
    hipLaunchKernelGGL((final_euler_kernel<AT, VEC>), dim3((F * T / VEC + 255) / 256, B), dim3(256), (size_t)3 * C * sizeof(float), st,
                       (const AT *)raw, sc, sh, w, bias, mask, C, F, T, est_out, xt, mu, noise, beta, h, sqrtf(beta * h), v);
    return hipGetLastError();
}
hipError_t launch_final_euler(const void *raw, const float *sc, const float *sh, const float *w, const float *bias,
                              const float *mask, int B, int C, int F, int T, float *est_out, float *xt, const float *mu,
                              const float *noise, float beta, float h, hipStream_t st, const VcStep *vc, int act_bf16, std::string *name) {
    VcStep v;
    v.mode = 0; v.cm = v.k1 = v.bh = v.sigma = 0.f;
    if (vc) v = *vc;
    if (act_bf16 && T % 4 == 0)
        return launch_final_euler_t<__bf16, 4>(raw, sc, sh, w, bias, mask, B, C, F, T, est_out, xt, mu, noise, beta, h, st, v, name);
    if (act_bf16)
        return launch_final_euler_t<__bf16, 1>(raw, sc, sh, w, bias, mask, B, C, F, T, est_out, xt, mu, noise, beta, h, st, v, name);
    return launch_final_euler_t<float, 1>(raw, sc, sh, w, bias, mask, B, C, F, T, est_out, xt, mu, noise, beta, h, st, v, name);
}

}  // namespace gtts
