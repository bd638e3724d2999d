// enc_train.hip -- TRAINING of the encoders' two fp32 VALU ops (enc.hip holds their inference kernels, which this file does not touch):
//   the windowed relative-position attention core of MultiHeadAttention.attention (Grad-TTS/model/text_encoder.py:145-175), forward
//   with dropout and backward, and the backward of LayerNorm over channels with the five flags of gtts_enc_layernorm.
// Nothing L x L is kept between forward and backward: the forward leaves per query row its score maximum and the reciprocal of its
// exponential sum (`stat`), and the backward recomputes  p_ij = expf(s_ij - max_i) * rs_i  through the SAME device functions
// (enct_dot / enct_score / enct_prob, implicit contraction off) the forward used, so the recomputed probabilities are the forward's
// bit for bit.  With  s the masked scores, p the softmax, pd = p * drop, r = j - i + w, inv = 1 / sqrt(dk):
//   dpd_ij = dout_i . v_j + [|j-i| <= w] dout_i . Ev[r]          dv_j   = sum_i pd_ij dout_i        dEv[r] = sum_{b,h,i} pd_{i,i+r-w} dout_i
//   dp = dpd * drop        delta_i = sum_j p_ij dp_ij            ds_ij  = p_ij (dp_ij - delta_i), 0 where the score was filled with -1e4
//   dq_i = inv sum_j ds_ij (k_j + [band] Ek[r])                  dk_j   = inv sum_i ds_ij q_i       dEk[r] = inv sum_{b,h,i} ds_{i,i+r-w} q_i
// Four launches:  (1) query-tiled (8 queries per workgroup): p, dp, delta, ds in LDS -> dq, delta and the band entries of ds / pd to
// scratch;  (2) key-tiled (64 keys per workgroup, every query tile in ascending order): dk, dv accumulated per (key, channel) by one
// thread -- no sum across workgroups;  (3) band: dEk / dEv partials per group of (b, h) items;  (4) fold of the partials in ascending
// order.  No floating-point atomics anywhere: two calls on the same inputs give the same bits.
// Layout [B][C][t] fp32, t fastest; head h = channels [h dk, (h + 1) dk).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/gradtts_abi.h"
#include "common.h"
#include "kernels.h"

namespace gtts {

// ---- the one spelling of a score and of a probability (forward and both backward passes)
// acc[qi] = sum_d a[d][qi] g[d] as ONE fmaf chain over d = 0 .. dk - 1 per query; a: LDS [dk][stride] (16-byte aligned rows), g: the
// key's column (stride gs floats between channels: L in global memory, 64 in an LDS tile)
template <int NQ>
__device__ __forceinline__ void enct_dot(const float *a, int stride, const float *g, size_t gs, int dk, float (&acc)[NQ]) {
    static_assert(NQ % 4 == 0, "queries in float4 groups");
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) acc[qi] = 0.f;
    for (int d = 0; d < dk; ++d) {
        const float kv = g[(size_t)d * gs];
        const float4 *a4 = reinterpret_cast<const float4 *>(a + d * stride);
#pragma unroll
        for (int u = 0; u < NQ / 4; ++u) {
            const float4 qq = a4[u];
            acc[4 * u + 0] = fmaf(qq.x, kv, acc[4 * u + 0]);
            acc[4 * u + 1] = fmaf(qq.y, kv, acc[4 * u + 1]);
            acc[4 * u + 2] = fmaf(qq.z, kv, acc[4 * u + 2]);
            acc[4 * u + 3] = fmaf(qq.w, kv, acc[4 * u + 3]);
        }
    }
}
// a_qi . E[r] for the relative embeddings: one fmaf chain over d
__device__ __forceinline__ float enct_rel(const float *a, int stride, int qi, const float *e, int dk) {
    float ar = 0.f;
    for (int d = 0; d < dk; ++d) ar = fmaf(a[d * stride + qi], e[d], ar);
    return ar;
}
__device__ __forceinline__ float enct_score(float dot, float rel, bool band, float inv, bool dead) {
#pragma clang fp contract(off)
    float sc = dot * inv;
    if (band) sc = sc + rel * inv;
    return dead ? -1e4f : sc;
}
__device__ __forceinline__ float enct_prob(float sc, float mx, float rs) {
#pragma clang fp contract(off)
    const float e = expf(sc - mx);
    return e * rs;
}

// o[d][qi] = sum_j w[qi][j] g[d][j] over all L keys, lanes along the keys (coalesced rows of g), 64 / QT channels per pass and wave;
// fin(d, qi, total) runs in the lane that owns (d, qi).  w: LDS [QT][LP]; entries j >= L are never read.
template <int QT, typename F>
__device__ __forceinline__ void enct_rows_times(const float *w, int LP, const float *g, int dk, int L, int wave, int lane, F fin) {
    constexpr int DD = 64 / QT;
    const int nblk = LP / 64;
    for (int dg = wave; dg * DD < dk; dg += 4) {                    // wave-uniform
        float acc[DD][QT];
#pragma unroll
        for (int dd = 0; dd < DD; ++dd)
#pragma unroll
            for (int qi = 0; qi < QT; ++qi) acc[dd][qi] = 0.f;
        for (int jb = 0; jb < nblk; ++jb) {
            const int j = jb * 64 + lane;
            const bool valid = j < L;
            const int jc = valid ? j : L - 1;
            float vv[DD], pp[QT];
#pragma unroll
            for (int dd = 0; dd < DD; ++dd) {
                const int d = min(dg * DD + dd, dk - 1);
                vv[dd] = valid ? g[(size_t)d * L + jc] : 0.f;
            }
#pragma unroll
            for (int qi = 0; qi < QT; ++qi) pp[qi] = valid ? w[(size_t)qi * LP + j] : 0.f;
#pragma unroll
            for (int dd = 0; dd < DD; ++dd)
#pragma unroll
                for (int qi = 0; qi < QT; ++qi) acc[dd][qi] = fmaf(pp[qi], vv[dd], acc[dd][qi]);
        }
        float mine = 0.f;
#pragma unroll
        for (int dd = 0; dd < DD; ++dd)
#pragma unroll
            for (int qi = 0; qi < QT; ++qi) {
                const float tot = wave_sum(acc[dd][qi]);            // (every lane gets the total)
                if (lane == dd * QT + qi) mine = tot;
            }
        const int d = dg * DD + lane / QT;
        if (d < dk) fin(d, lane % QT, mine);
    }
}

// ================================================================================================ attention forward (training)
// One workgroup per (16 queries, head, sample), lanes along the keys.  LDS: [dk][16] queries, [16][2w+1] q . Ek, [16][roundup(L, 64)]
// scores -> probabilities -> p * drop, [16] query masks.
constexpr int TF_QT = 16;
__global__ __launch_bounds__(256) void enc_att_train_fwd_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                                const float *__restrict__ v, const float *__restrict__ mask,
                                                                const float *__restrict__ ek, const float *__restrict__ ev,
                                                                const float *__restrict__ drop, float *__restrict__ out,
                                                                float *__restrict__ stat, int C, int L, int heads, int win) {
    constexpr int QT = TF_QT;
    extern __shared__ float sm[];
    const int dk = C / heads, LP = (L + 63) / 64 * 64, nr = win > 0 ? 2 * win + 1 : 0;
    float *s_q = sm;                          // [dk][QT]
    float *s_rel = s_q + dk * QT;             // [QT][nr]
    float *s_p = s_rel + QT * nr;             // [QT][LP]
    float *s_mi = s_p + (size_t)QT * LP;      // [QT]
    const int b = blockIdx.z, h = blockIdx.y, i0 = blockIdx.x * QT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t hb = ((size_t)b * C + (size_t)h * dk) * L, bh = (size_t)b * heads + h;
    const float *qb = q + hb, *kb = k + hb, *vb = v + hb, *mb = mask + (size_t)b * L;
    const float inv = 1.0f / sqrtf((float)dk);
    for (int e = tid; e < QT * dk; e += 256) {
        const int d = e / QT, qi = e - d * QT;
        s_q[e] = i0 + qi < L ? qb[(size_t)d * L + i0 + qi] : 0.f;
    }
    if (tid < QT) s_mi[tid] = mb[min(i0 + tid, L - 1)];
    __syncthreads();
    for (int e = tid; e < QT * nr; e += 256) {
        const int qi = e / nr, r = e - qi * nr;
        s_rel[e] = enct_rel(s_q, QT, qi, ek + (size_t)r * dk, dk);
    }
    __syncthreads();
    const int nblk = LP / 64;
    for (int jb = wave; jb < nblk; jb += 4) {
        const int j = jb * 64 + lane;
        const bool valid = j < L;
        const int jc = valid ? j : L - 1;
        float acc[QT];
        enct_dot<QT>(s_q, QT, kb + jc, (size_t)L, dk, acc);
        const float mj = mb[jc];
#pragma unroll
        for (int qi = 0; qi < QT; ++qi) {
            const int r = j - (i0 + qi) + win;
            const bool band = nr > 0 && r >= 0 && r < nr;
            const float sc = enct_score(acc[qi], band ? s_rel[qi * nr + r] : 0.f, band, inv, s_mi[qi] * mj == 0.f);
            if (valid) s_p[(size_t)qi * LP + j] = sc;
        }
    }
    __syncthreads();
    for (int qq = 0; qq < QT / 4; ++qq) {
        const int qi = wave * (QT / 4) + qq, i = i0 + qi;
        if (i >= L) continue;                                       // wave-uniform
        float *pv = s_p + (size_t)qi * LP;
        float mx = -INFINITY;
        for (int j = lane; j < L; j += 64) mx = fmaxf(mx, pv[j]);
        mx = wave_max(mx);
        float sum = 0.f;
        for (int j = lane; j < L; j += 64) sum += expf(pv[j] - mx);
        sum = wave_sum(sum);
        const float rs = 1.0f / sum;
        if (lane == 0) {
            stat[(bh * L + i) * 2 + 0] = mx;
            stat[(bh * L + i) * 2 + 1] = rs;
        }
        const float *dr = drop ? drop + (bh * L + i) * L : nullptr;
        for (int j = lane; j < L; j += 64) {
            float p = enct_prob(pv[j], mx, rs);
            if (dr) p *= dr[j];
            pv[j] = p;
        }
    }
    __syncthreads();
    enct_rows_times<QT>(s_p, LP, vb, dk, L, wave, lane, [&](int d, int qi, float o) {
        const int i = i0 + qi;
        if (i >= L) return;
        const float *pv = s_p + (size_t)qi * LP;
        for (int r = 0; r < nr; ++r) {
            const int j = i + r - win;
            if (j >= 0 && j < L) o = fmaf(pv[j], ev[r * dk + d], o);
        }
        out[hb + (size_t)d * L + i] = o;
    });
}

// ================================================================================================ attention backward, query-tiled
// One workgroup per (8 queries, head, sample).  LDS: [dk][8] q and dout, [8][2w+1] q . Ek and dout . Ev, [8][LP] p and dp -> ds,
// [4][8] row constants.  Writes dq, delta [B][H][L] and the band entries dsb / pdb [B][H][2w+1][L] (index [r][i]: ds / pd at (i, i + r - w)).
constexpr int TA_QT = 8;
__global__ __launch_bounds__(256) void enc_att_train_bwd_q_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                                  const float *__restrict__ v, const float *__restrict__ mask,
                                                                  const float *__restrict__ ek, const float *__restrict__ ev,
                                                                  const float *__restrict__ drop, const float *__restrict__ stat,
                                                                  const float *__restrict__ dout, float *__restrict__ dq,
                                                                  float *__restrict__ delta, float *__restrict__ dsb,
                                                                  float *__restrict__ pdb, int C, int L, int heads, int win) {
    constexpr int QT = TA_QT;
    extern __shared__ float sm[];
    const int dk = C / heads, LP = (L + 63) / 64 * 64, nr = win > 0 ? 2 * win + 1 : 0;
    float *s_q = sm;                          // [dk][QT]
    float *s_do = s_q + dk * QT;              // [dk][QT]
    float *s_rk = s_do + dk * QT;             // [QT][nr]
    float *s_rv = s_rk + QT * nr;             // [QT][nr]
    float *s_p = s_rv + QT * nr;              // [QT][LP]
    float *s_dp = s_p + (size_t)QT * LP;      // [QT][LP]
    float *s_row = s_dp + (size_t)QT * LP;    // [4][QT]: max, 1 / sum, query mask, delta
    const int b = blockIdx.z, h = blockIdx.y, i0 = blockIdx.x * QT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t hb = ((size_t)b * C + (size_t)h * dk) * L, bh = (size_t)b * heads + h;
    const float *qb = q + hb, *kb = k + hb, *vb = v + hb, *gb = dout + hb, *mb = mask + (size_t)b * L;
    const float inv = 1.0f / sqrtf((float)dk);
    for (int e = tid; e < QT * dk; e += 256) {
        const int d = e / QT, qi = e - d * QT;
        const bool in = i0 + qi < L;
        s_q[e] = in ? qb[(size_t)d * L + i0 + qi] : 0.f;
        s_do[e] = in ? gb[(size_t)d * L + i0 + qi] : 0.f;
    }
    if (tid < QT) {
        const int ic = min(i0 + tid, L - 1);
        s_row[0 * QT + tid] = stat[(bh * L + ic) * 2 + 0];
        s_row[1 * QT + tid] = stat[(bh * L + ic) * 2 + 1];
        s_row[2 * QT + tid] = mb[ic];
    }
    __syncthreads();
    for (int e = tid; e < QT * nr; e += 256) {
        const int qi = e / nr, r = e - qi * nr;
        s_rk[e] = enct_rel(s_q, QT, qi, ek + (size_t)r * dk, dk);
        s_rv[e] = enct_rel(s_do, QT, qi, ev + (size_t)r * dk, dk);
    }
    __syncthreads();
    const int nblk = LP / 64;
    for (int jb = wave; jb < nblk; jb += 4) {
        const int j = jb * 64 + lane;
        const bool valid = j < L;
        const int jc = valid ? j : L - 1;
        float as[QT], av[QT];
        enct_dot<QT>(s_q, QT, kb + jc, (size_t)L, dk, as);
        enct_dot<QT>(s_do, QT, vb + jc, (size_t)L, dk, av);
        const float mj = mb[jc];
#pragma unroll
        for (int qi = 0; qi < QT; ++qi) {
            const int i = i0 + qi, r = j - i + win;
            const bool band = nr > 0 && r >= 0 && r < nr;
            if (!valid || i >= L) continue;
            const float sc = enct_score(as[qi], band ? s_rk[qi * nr + r] : 0.f, band, inv, s_row[2 * QT + qi] * mj == 0.f);
            const float p = enct_prob(sc, s_row[0 * QT + qi], s_row[1 * QT + qi]);
            const float dm = drop ? drop[(bh * L + i) * L + j] : 1.f;
            const float dpd = band ? av[qi] + s_rv[qi * nr + r] : av[qi];
            s_p[(size_t)qi * LP + j] = p;
            s_dp[(size_t)qi * LP + j] = dpd * dm;
            if (band) pdb[(bh * nr + r) * L + i] = p * dm;
        }
    }
    __syncthreads();
    for (int qq = 0; qq < QT / 4; ++qq) {
        const int qi = wave * (QT / 4) + qq, i = i0 + qi;
        if (i >= L) continue;                                       // wave-uniform
        const float *pv = s_p + (size_t)qi * LP;
        float *dv = s_dp + (size_t)qi * LP;
        float dl = 0.f;
        for (int j = lane; j < L; j += 64) dl = fmaf(pv[j], dv[j], dl);
        dl = wave_sum(dl);
        if (lane == 0) delta[bh * L + i] = dl;
        const float mi = s_row[2 * QT + qi];
        for (int j = lane; j < L; j += 64) {
            const float ds = mi * mb[j] == 0.f ? 0.f : pv[j] * (dv[j] - dl);
            dv[j] = ds;
            const int r = j - i + win;
            if (nr > 0 && r >= 0 && r < nr) dsb[(bh * nr + r) * L + i] = ds;
        }
    }
    __syncthreads();
    enct_rows_times<QT>(s_dp, LP, kb, dk, L, wave, lane, [&](int d, int qi, float o) {
        const int i = i0 + qi;
        if (i >= L) return;
        const float *dv = s_dp + (size_t)qi * LP;
        for (int r = 0; r < nr; ++r) {
            const int j = i + r - win;
            if (j >= 0 && j < L) o = fmaf(dv[j], ek[r * dk + d], o);
        }
        dq[hb + (size_t)d * L + i] = o * inv;
    });
}

// ================================================================================================ attention backward, key-tiled
// One workgroup per (64 keys, head, sample), lane = key; it walks every 16-query tile in ascending order, recomputes p, pd and ds of
// the 16 x 64 block (a wave per four queries) and adds the block's terms to dk / dv, held in LDS as [dk][64] accumulators that one
// thread per (channel, key) owns: the sum over queries has one fixed order and crosses no workgroup.
constexpr int TB_QT = 16, TB_KT = 64;
__global__ __launch_bounds__(256) void enc_att_train_bwd_k_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                                  const float *__restrict__ v, const float *__restrict__ mask,
                                                                  const float *__restrict__ ek, const float *__restrict__ ev,
                                                                  const float *__restrict__ drop, const float *__restrict__ stat,
                                                                  const float *__restrict__ dout, const float *__restrict__ delta,
                                                                  float *__restrict__ dkey, float *__restrict__ dval, int C, int L,
                                                                  int heads, int win) {
    constexpr int QT = TB_QT, KT = TB_KT;
    extern __shared__ float sm[];
    const int dk = C / heads, nr = win > 0 ? 2 * win + 1 : 0;
    float *s_k = sm;                          // [dk][KT]
    float *s_v = s_k + dk * KT;               // [dk][KT]
    float *s_ak = s_v + dk * KT;              // [dk][KT] accumulators of dk
    float *s_av = s_ak + dk * KT;             // [dk][KT] accumulators of dv
    float *s_q = s_av + dk * KT;              // [dk][QT]
    float *s_do = s_q + dk * QT;              // [dk][QT]
    float *s_pd = s_do + dk * QT;             // [QT][KT]
    float *s_ds = s_pd + QT * KT;             // [QT][KT]
    float *s_row = s_ds + QT * KT;            // [4][QT]: max, 1 / sum, query mask, delta
    float *s_rk = s_row + 4 * QT;             // [QT][nr]
    float *s_rv = s_rk + QT * nr;             // [QT][nr]
    const int b = blockIdx.z, h = blockIdx.y, j0 = blockIdx.x * KT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t hb = ((size_t)b * C + (size_t)h * dk) * L, bh = (size_t)b * heads + h;
    const float *qb = q + hb, *kb = k + hb, *vb = v + hb, *gb = dout + hb, *mb = mask + (size_t)b * L;
    const float inv = 1.0f / sqrtf((float)dk);
    const int j = j0 + lane;
    const bool valid = j < L;
    const int jc = valid ? j : L - 1;
    for (int e = tid; e < dk * KT; e += 256) {
        const int d = e / KT, jj = min(j0 + (e - d * KT), L - 1);
        s_k[e] = kb[(size_t)d * L + jj];
        s_v[e] = vb[(size_t)d * L + jj];
        s_ak[e] = 0.f;
        s_av[e] = 0.f;
    }
    const float mj = mb[jc];
    for (int i0 = 0; i0 < L; i0 += QT) {
        __syncthreads();                                            // the previous tile's readers are done (and the tiles above are loaded)
        for (int e = tid; e < QT * dk; e += 256) {
            const int d = e / QT, qi = e - d * QT;
            const bool in = i0 + qi < L;
            s_q[e] = in ? qb[(size_t)d * L + i0 + qi] : 0.f;
            s_do[e] = in ? gb[(size_t)d * L + i0 + qi] : 0.f;
        }
        if (tid < QT) {
            const int ic = min(i0 + tid, L - 1);
            s_row[0 * QT + tid] = stat[(bh * L + ic) * 2 + 0];
            s_row[1 * QT + tid] = stat[(bh * L + ic) * 2 + 1];
            s_row[2 * QT + tid] = mb[ic];
            s_row[3 * QT + tid] = delta[bh * L + ic];
        }
        __syncthreads();
        // (workgroup-uniform) does the band |j - i| <= w cross this 16 x 64 block at all?
        const bool near = nr > 0 && i0 + QT - 1 + win >= j0 && i0 - win <= j0 + KT - 1;
        if (near) {
            for (int e = tid; e < QT * nr; e += 256) {
                const int qi = e / nr, r = e - qi * nr;
                s_rk[e] = enct_rel(s_q, QT, qi, ek + (size_t)r * dk, dk);
                s_rv[e] = enct_rel(s_do, QT, qi, ev + (size_t)r * dk, dk);
            }
            __syncthreads();
        }
        float as[4], av[4];
        enct_dot<4>(s_q + 4 * wave, QT, s_k + lane, (size_t)KT, dk, as);
        enct_dot<4>(s_do + 4 * wave, QT, s_v + lane, (size_t)KT, dk, av);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int qi = 4 * wave + c, i = i0 + qi;
            float pd = 0.f, ds = 0.f;
            if (valid && i < L) {
                const int r = j - i + win;
                const bool band = near && r >= 0 && r < nr;
                const bool dead = s_row[2 * QT + qi] * mj == 0.f;
                const float sc = enct_score(as[c], band ? s_rk[qi * nr + r] : 0.f, band, inv, dead);
                const float p = enct_prob(sc, s_row[0 * QT + qi], s_row[1 * QT + qi]);
                const float dm = drop ? drop[(bh * L + i) * L + j] : 1.f;
                const float dpd = band ? av[c] + s_rv[qi * nr + r] : av[c];
                pd = p * dm;
                ds = dead ? 0.f : p * (dpd * dm - s_row[3 * QT + qi]);
            }
            s_pd[qi * KT + lane] = pd;
            s_ds[qi * KT + lane] = ds;
        }
        __syncthreads();
        float pr[QT], dr[QT];
#pragma unroll
        for (int qi = 0; qi < QT; ++qi) {
            pr[qi] = s_pd[qi * KT + lane];
            dr[qi] = s_ds[qi * KT + lane];
        }
        for (int d = wave; d < dk; d += 4) {
            const float4 *g4 = reinterpret_cast<const float4 *>(s_do + d * QT), *q4 = reinterpret_cast<const float4 *>(s_q + d * QT);
            float a = s_av[d * KT + lane], c = s_ak[d * KT + lane];
#pragma unroll
            for (int u = 0; u < QT / 4; ++u) {
                const float4 g = g4[u], qq = q4[u];
                a = fmaf(pr[4 * u + 0], g.x, a);
                a = fmaf(pr[4 * u + 1], g.y, a);
                a = fmaf(pr[4 * u + 2], g.z, a);
                a = fmaf(pr[4 * u + 3], g.w, a);
                c = fmaf(dr[4 * u + 0], qq.x, c);
                c = fmaf(dr[4 * u + 1], qq.y, c);
                c = fmaf(dr[4 * u + 2], qq.z, c);
                c = fmaf(dr[4 * u + 3], qq.w, c);
            }
            s_av[d * KT + lane] = a;
            s_ak[d * KT + lane] = c;
        }
    }
    if (!valid) return;
    for (int d = wave; d < dk; d += 4) {                            // (each thread reads back the accumulators it owns)
        dval[hb + (size_t)d * L + j] = s_av[d * KT + lane];
        dkey[hb + (size_t)d * L + j] = s_ak[d * KT + lane] * inv;
    }
}

// ================================================================================================ relative embeddings' gradients
// partial[g][0][r][d] = sum_{bh = g, g + G, ...} sum_i dsb[bh][r][i] q[bh][d][i],  partial[g][1][r][d] the same of pdb and dout.
// Grid (2w+1, G); a wave per channel, lanes along i.  The (i, i + r - w) pairs outside the sequence were never written: skipped.
__global__ __launch_bounds__(256) void enc_att_train_band_kernel(const float *__restrict__ q, const float *__restrict__ dout,
                                                                 const float *__restrict__ dsb, const float *__restrict__ pdb,
                                                                 float *__restrict__ partial, int C, int L, int heads, int BH, int G,
                                                                 int win) {
    const int r = blockIdx.x, g = blockIdx.y, nr = gridDim.x, dk = C / heads;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int d = wave; d < dk; d += 4) {
        float ak = 0.f, av = 0.f;
        for (int bh = g; bh < BH; bh += G) {
            const int b = bh / heads, h = bh - b * heads;
            const size_t base = ((size_t)b * C + (size_t)h * dk + d) * L, row = ((size_t)bh * nr + r) * L;
            for (int i = lane; i < L; i += 64) {
                const int j = i + r - win;
                if (j < 0 || j >= L) continue;
                ak = fmaf(dsb[row + i], q[base + i], ak);
                av = fmaf(pdb[row + i], dout[base + i], av);
            }
        }
        ak = wave_sum(ak);
        av = wave_sum(av);
        if (lane == 0) {
            partial[(((size_t)g * 2 + 0) * nr + r) * dk + d] = ak;
            partial[(((size_t)g * 2 + 1) * nr + r) * dk + d] = av;
        }
    }
}
__global__ void enc_att_train_fold_kernel(const float *__restrict__ partial, float *__restrict__ dek, float *__restrict__ dev, int n,
                                          int G, float inv) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * n) return;
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += partial[(size_t)g * 2 * n + e];          // ascending g: one fixed order
    if (e < n) dek[e] = s * inv;
    else dev[e - n] = s;
}

// ================================================================================================ LayerNorm backward
// The forward's geometry (16 positions x 16 channel lanes per workgroup) and its two-pass mean / rstd, recomputed from the inputs;
//   g = dout * out_mask, 0 where relu_out clipped;  dxhat = g gamma;  dv = rstd (dxhat - mean_c dxhat - xhat mean_c (dxhat xhat));
//   dbres = dv;  da = dv * a_mask * [a > 0 under relu_in];  per-workgroup partials of dgamma = sum g xhat and dbeta = sum g.
__global__ __launch_bounds__(256) void enc_layernorm_bwd_kernel(const float *__restrict__ dout, const float *__restrict__ a,
                                                                const float *__restrict__ bres, const float *__restrict__ gamma,
                                                                const float *__restrict__ beta, const float *__restrict__ a_mask,
                                                                const float *__restrict__ out_mask, float *__restrict__ da,
                                                                float *__restrict__ dbres, float *__restrict__ partial, int C, int L,
                                                                float eps, int relu_in, int relu_out) {
    // no implicit mul+add fusion: `dxhat - mean(dxhat)` must see the ROUNDED product g * gamma that the mean was summed from (fused, a
    // single-channel LayerNorm's gradient would be the product's rounding residue instead of an exact zero)
#pragma clang fp contract(off)
    __shared__ float s_red[4][4][16];
    const int b = blockIdx.y, tl = threadIdx.x & 15, cl = threadIdx.x >> 4, wave = threadIdx.x >> 6;
    const int t = blockIdx.x * 16 + tl;
    const bool ok = t < L;
    const int tc = ok ? t : L - 1;
    const size_t base = (size_t)b * C * L + tc;
    const float am = a_mask ? a_mask[(size_t)b * L + tc] : 1.f;
    const float om = out_mask ? out_mask[(size_t)b * L + tc] : 1.f;
    auto val = [&](int c) {
        float x = a[base + (size_t)c * L];
        if (relu_in) x = fmaxf(x, 0.f);
        x *= am;
        if (bres) x += bres[base + (size_t)c * L];
        return x;
    };
    auto reduce16 = [&](float x, int slot) {                 // sum over the 16 channel lanes of this thread's position
        x += __shfl_xor(x, 16, 64);
        x += __shfl_xor(x, 32, 64);
        if ((threadIdx.x & 48) == 0) s_red[slot][wave][tl] = x;
        __syncthreads();
        return (s_red[slot][0][tl] + s_red[slot][1][tl]) + (s_red[slot][2][tl] + s_red[slot][3][tl]);
    };
    float s = 0.f;
    for (int c = cl; c < C; c += 16) s += val(c);
    const float mean = reduce16(s, 0) / (float)C;
    float qd = 0.f;
    for (int c = cl; c < C; c += 16) {
        const float d = val(c) - mean;
        qd = fmaf(d, d, qd);
    }
    const float rstd = rsqrtf(reduce16(qd, 1) / (float)C + eps);
    auto grad = [&](int c, float xh) {                       // dL / d(xhat gamma + beta)
        float g = ok ? dout[base + (size_t)c * L] * om : 0.f;
        if (relu_out && !(fmaf(xh, gamma[c], beta[c]) > 0.f)) g = 0.f;
        return g;
    };
    float *part = partial + ((size_t)b * gridDim.x + blockIdx.x) * 2 * C;
    float s1 = 0.f, s2 = 0.f;
    for (int c = cl; c < C; c += 16) {
        const float xh = (val(c) - mean) * rstd, g = grad(c, xh), dx = g * gamma[c];
        s1 += dx;
        s2 = fmaf(dx, xh, s2);
        float pg = g * xh, pb = g;                           // over the tile's 16 positions (lane bits 0-3)
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            pg += __shfl_xor(pg, m, 64);
            pb += __shfl_xor(pb, m, 64);
        }
        if (tl == 0) {
            part[c] = pg;
            part[C + c] = pb;
        }
    }
    const float m1 = reduce16(s1, 2) / (float)C, m2 = reduce16(s2, 3) / (float)C;
    if (!ok) return;
    for (int c = cl; c < C; c += 16) {
        const float xh = (val(c) - mean) * rstd, dx = grad(c, xh) * gamma[c];
        const float dv = rstd * (dx - m1 - xh * m2);
        if (dbres) dbres[base + (size_t)c * L] = dv;
        float t0 = dv * am;
        if (relu_in && !(a[base + (size_t)c * L] > 0.f)) t0 = 0.f;
        da[base + (size_t)c * L] = t0;
    }
}
// dgamma[c] / dbeta[c] = the workgroups' partials in ascending order (four interleaved chains, combined in one fixed tree)
__global__ void enc_layernorm_fold_kernel(const float *__restrict__ partial, float *__restrict__ dgamma, float *__restrict__ dbeta,
                                          int C, int nwg) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * C) return;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int w = 0;
    for (; w + 4 <= nwg; w += 4)
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] += partial[(size_t)(w + u) * 2 * C + e];
    for (int u = 0; w + u < nwg; ++u) s[u] += partial[(size_t)(w + u) * 2 * C + e];
    const float tot = (s[0] + s[1]) + (s[2] + s[3]);
    if (e < C) dgamma[e] = tot;
    else dbeta[e - C] = tot;
}

}  // namespace gtts

using namespace gtts;

// ---- dynamic LDS of the three attention kernels, in bytes (include/gradtts_abi.h restates them)
constexpr size_t ENCT_LDS_LIMIT = (size_t)160 * 1024;
static inline size_t enct_nr(int window) { return window > 0 ? 2 * (size_t)window + 1 : 0; }
static inline size_t enct_lp(int L) { return ((size_t)L + 63) / 64 * 64; }
static inline size_t enct_fwd_lds(int dk, int window, int L) {
    return ((size_t)dk * TF_QT + TF_QT * enct_nr(window) + TF_QT * enct_lp(L) + TF_QT) * sizeof(float);
}
static inline size_t enct_bwd_q_lds(int dk, int window, int L) {
    return (2 * (size_t)dk * TA_QT + 2 * TA_QT * enct_nr(window) + 2 * TA_QT * enct_lp(L) + 4 * TA_QT) * sizeof(float);
}
static inline size_t enct_bwd_k_lds(int dk, int window) {
    return (4 * (size_t)dk * TB_KT + 2 * (size_t)dk * TB_QT + 2 * TB_QT * TB_KT + 4 * TB_QT + 2 * TB_QT * enct_nr(window)) * sizeof(float);
}
static bool enct_config_ok(int channels, int n_heads, int window) {
    return channels > 0 && n_heads > 0 && channels % n_heads == 0 && window >= 0;
}
static bool enct_width_ok(int dk, int window) {                     // what no length can fix
    return window <= (1 << 20) && dk <= (1 << 20) && enct_bwd_k_lds(dk, window) <= ENCT_LDS_LIMIT && enct_fwd_lds(dk, window, 1) <= ENCT_LDS_LIMIT &&
           enct_bwd_q_lds(dk, window, 1) <= ENCT_LDS_LIMIT;
}
static int enct_ok(int channels, int n_heads, int window, int L) {
    if (!enct_config_ok(channels, n_heads, window) || L <= 0 || L > (1 << 24)) return 0;
    const int dk = channels / n_heads;
    return enct_width_ok(dk, window) && enct_fwd_lds(dk, window, L) <= ENCT_LDS_LIMIT && enct_bwd_q_lds(dk, window, L) <= ENCT_LDS_LIMIT;
}
extern "C" int gtts_enc_attention_train_ok(int channels, int n_heads, int window, int L) { return enct_ok(channels, n_heads, window, L); }

static int enct_groups(int BH) { return BH < 32 ? BH : 32; }
// scratch of the backward, in floats: delta [B H L], dsb and pdb [B H (2w+1) L], partial [G][2][2w+1][dk]
extern "C" size_t gtts_enc_attention_train_scratch_bytes(int B, int C, int L, int n_heads, int window) {
    if (B <= 0 || B > 65535 || n_heads > 65535 || !enct_ok(C, n_heads, window, L)) return 0;
    const size_t BH = (size_t)B * n_heads, nr = enct_nr(window), dk = (size_t)(C / n_heads);
    return (BH * L + 2 * BH * nr * L + (size_t)enct_groups((int)BH) * 2 * nr * dk) * sizeof(float);
}

// Everything that can be refused is refused here, on the host, before the first HIP call.
static int enct_check(const char *who, int B, int C, int L, int heads, int window) {
    if (B <= 0 || L <= 0) return fail(GTTS_E_SHAPE, "%s: bad shape B=%d L=%d", who, B, L);
    if (!enct_config_ok(C, heads, window)) return fail(GTTS_E_CONFIG, "%s: unsupported channels=%d n_heads=%d window=%d", who, C, heads, window);
    if (B > 65535 || heads > 65535) return fail(GTTS_E_SHAPE, "%s: B=%d / n_heads=%d exceed the launch grid", who, B, heads);
    if (!enct_width_ok(C / heads, window))
        return fail(GTTS_E_CONFIG, "%s: head width %d with window %d does not fit the training kernels' LDS", who, C / heads, window);
    if (!enct_ok(C, heads, window, L)) return fail(GTTS_E_SHAPE, "%s: sequence too long for the training attention kernels (%d)", who, L);
    return GTTS_OK;
}

extern "C" int gtts_enc_attention_train_forward(const float *q, const float *k, const float *v, const float *mask, const float *emb_rel_k,
                                                const float *emb_rel_v, const float *drop, float *out, float *stat, int B, int C, int L,
                                                int n_heads, int window, gtts_stream_t stream) {
    if (!q || !k || !v || !mask || !out || !stat) return fail(GTTS_E_NULL, "gtts_enc_attention_train_forward: null argument");
    if (window > 0 && (!emb_rel_k || !emb_rel_v))
        return fail(GTTS_E_NULL, "gtts_enc_attention_train_forward: a window needs emb_rel_k and emb_rel_v");
    if (int rc = enct_check("gtts_enc_attention_train_forward", B, C, L, n_heads, window)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t smem = enct_fwd_lds(C / n_heads, window, L);
    GTTS_HIPCHK(raise_dyn_lds<&enc_att_train_fwd_kernel>(smem));
    hipLaunchKernelGGL(enc_att_train_fwd_kernel, dim3((L + TF_QT - 1) / TF_QT, n_heads, B), dim3(256), smem, st, q, k, v, mask, emb_rel_k,
                       emb_rel_v, drop, out, stat, C, L, n_heads, window);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}

extern "C" int gtts_enc_attention_train_backward(const float *q, const float *k, const float *v, const float *mask, const float *emb_rel_k,
                                                 const float *emb_rel_v, const float *drop, const float *stat, const float *dout, float *dq,
                                                 float *dk, float *dv, float *dek, float *dev, void *scratch, int B, int C, int L,
                                                 int n_heads, int window, gtts_stream_t stream) {
    if (!q || !k || !v || !mask || !stat || !dout || !dq || !dk || !dv || !scratch)
        return fail(GTTS_E_NULL, "gtts_enc_attention_train_backward: null argument");
    if (window > 0 && (!emb_rel_k || !emb_rel_v || !dek || !dev))
        return fail(GTTS_E_NULL, "gtts_enc_attention_train_backward: a window needs emb_rel_k, emb_rel_v and their gradients");
    if (int rc = enct_check("gtts_enc_attention_train_backward", B, C, L, n_heads, window)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int dkw = C / n_heads, BH = B * n_heads, G = enct_groups(BH), nr = (int)enct_nr(window);
    float *delta = (float *)scratch, *dsb = delta + (size_t)BH * L, *pdb = dsb + (size_t)BH * nr * L, *partial = pdb + (size_t)BH * nr * L;
    const size_t smq = enct_bwd_q_lds(dkw, window, L), smk = enct_bwd_k_lds(dkw, window);
    GTTS_HIPCHK(raise_dyn_lds<&enc_att_train_bwd_q_kernel>(smq));
    GTTS_HIPCHK(raise_dyn_lds<&enc_att_train_bwd_k_kernel>(smk));
    hipLaunchKernelGGL(enc_att_train_bwd_q_kernel, dim3((L + TA_QT - 1) / TA_QT, n_heads, B), dim3(256), smq, st, q, k, v, mask, emb_rel_k,
                       emb_rel_v, drop, stat, dout, dq, delta, dsb, pdb, C, L, n_heads, window);
    GTTS_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(enc_att_train_bwd_k_kernel, dim3((L + TB_KT - 1) / TB_KT, n_heads, B), dim3(256), smk, st, q, k, v, mask, emb_rel_k,
                       emb_rel_v, drop, stat, dout, delta, dk, dv, C, L, n_heads, window);
    GTTS_HIPCHK(hipGetLastError());
    if (nr > 0) {
        hipLaunchKernelGGL(enc_att_train_band_kernel, dim3(nr, G), dim3(256), 0, st, q, dout, dsb, pdb, partial, C, L, n_heads, BH, G, window);
        GTTS_HIPCHK(hipGetLastError());
        const int n = nr * dkw;
        hipLaunchKernelGGL(enc_att_train_fold_kernel, dim3((2 * n + 255) / 256), dim3(256), 0, st, partial, dek, dev, n, G,
                           1.0f / sqrtf((float)dkw));
        GTTS_HIPCHK(hipGetLastError());
    }
    return GTTS_OK;
}

extern "C" size_t gtts_enc_layernorm_backward_scratch_floats(int B, int C, int L) {
    if (B <= 0 || C <= 0 || L <= 0 || B > 65535) return 0;
    return (size_t)B * ((L + 15) / 16) * 2 * C;
}
extern "C" int gtts_enc_layernorm_backward(const float *dout, const float *a, const float *bres, const float *gamma, const float *beta,
                                           const float *a_mask, const float *out_mask, float *da, float *dbres, float *dgamma, float *dbeta,
                                           float *scratch, int B, int C, int L, float eps, int relu_in, int relu_out, gtts_stream_t stream) {
    if (!dout || !a || !gamma || !beta || !da || !dgamma || !dbeta || !scratch)
        return fail(GTTS_E_NULL, "gtts_enc_layernorm_backward: null argument");
    if (bres && !dbres) return fail(GTTS_E_NULL, "gtts_enc_layernorm_backward: bres needs dbres");
    if (B <= 0 || C <= 0 || L <= 0 || B > 65535) return fail(GTTS_E_SHAPE, "gtts_enc_layernorm_backward: bad shape B=%d C=%d L=%d", B, C, L);
    if (!(eps > 0.f)) return fail(GTTS_E_CONFIG, "gtts_enc_layernorm_backward: eps must be positive");
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (L + 15) / 16;
    hipLaunchKernelGGL(enc_layernorm_bwd_kernel, dim3(tiles, B), dim3(256), 0, st, dout, a, bres, gamma, beta, a_mask, out_mask, da,
                       bres ? dbres : nullptr, scratch, C, L, eps, relu_in ? 1 : 0, relu_out ? 1 : 0);
    GTTS_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(enc_layernorm_fold_kernel, dim3((2 * C + 255) / 256), dim3(256), 0, st, scratch, dgamma, dbeta, C, tiles * B);
    GTTS_HIPCHK(hipGetLastError());
    return GTTS_OK;
}
