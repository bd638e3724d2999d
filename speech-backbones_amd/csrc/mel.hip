// mel.hip -- log-mel front end: waveform [B,L] -> log-mel [B,num_mels,T], the mel_spectrogram(..., center=False) of
// Grad-TTS/hifi-gan/meldataset.py:51-74 (DiffVC carries the same function) in ONE launch:
//   reflect pad (n_fft - hop)/2 -> frames of n_fft at stride hop -> periodic Hann window (zero-padded to n_fft) -> one-sided DFT
//   -> sqrt(re^2 + im^2 + 1e-9) -> slaney-normalised mel filterbank -> log(max(., 1e-5)).
// Layout: a workgroup of four waves owns a tile of MEL_TF = 16 consecutive frames of one row; every wave transforms four of them,
// one at a time, each frame by its own wave alone (no workgroup barrier inside a transform; the next frame's samples are loaded
// while the current one is transformed):
//   * the reflect padding and the framing are index arithmetic of the sample loads (no padded copy, no frame matrix);
//   * the n_fft real samples are packed as n_fft/2 complex points z[m] = x[2m] + i x[2m+1]; a Stockham autosort FFT (radix-4 passes,
//     one radix-2 pass when log2(n_fft/2) is odd) runs between two bank-swizzled LDS buffers of the wave, the lane's pass twiddles
//     held in registers; the real spectrum follows from
//     X[k] = E[k] + W_n^k O[k], E = (Z[k] + conj Z[M-k]) / 2, O = -i (Z[k] - conj Z[M-k]) / 2;
//   * twiddles, window and filterbank come from the packed table (host float64, gtts_mel_pack); no device sin / cos;
//   * only bins below the filterbank's last non-zero column are formed (372 of 513 at fmax = 8000); magnitudes stay in LDS;
//   * every mel row's support is a contiguous bin range, so the projection is one short dot product per (row, frame), in a fixed
//     order, with lanes along the frame axis -- the axis the [B,num_mels,T] store is contiguous in.
// A frame's value depends on its own n_fft samples and the tables alone: not on B, its place in the tile, or the grid.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/gradtts_abi.h"
#include "common.h"
#include "kernels.h"
#include "mel.h"
#include "spectral.h"

namespace gtts {

constexpr int MEL_TF = 16;         // frames per workgroup
constexpr int MEL_WAVES = 4;       // waves per workgroup; each transforms MEL_TF / MEL_WAVES frames

template <int LOGN>
__global__ __launch_bounds__(64 * MEL_WAVES) void mel_kernel(MelArgs a) {
    constexpr int N = 1 << LOGN, M = N / 2, Q = M / 4, R = M / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char mel_smem[];
    float2 *tw = reinterpret_cast<float2 *>(mel_smem);                       // [M]
    float2 *twn = tw + M;                                                    // [M + 2] (kmax used)
    float2 *bufs = twn + M + 2;                                              // [MEL_WAVES][2][M]
    float *mag = reinterpret_cast<float *>(bufs + MEL_WAVES * 2 * M);        // [MEL_TF][kstride]
    int4 *rows = reinterpret_cast<int4 *>(mag + ((MEL_TF * a.kstride + 3) & ~3));   // [num_mels]
    float *wts = reinterpret_cast<float *>(rows + a.num_mels);               // [nw]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * MEL_TF;
    int len = a.L;
    if (a.lengths) len = min(max(a.lengths[b], 0), a.L);
    const int Tb = min(mel_frames_of(len, N, a.hop, a.pad), a.T);
    float *out = a.out + (size_t)b * a.num_mels * a.T;
    if (t0 >= Tb) {                       // a tile behind the row's last frame: zeros (how the reference collate functions pad)
        for (int idx = tid; idx < a.num_mels * MEL_TF; idx += 64 * MEL_WAVES) {
            const int t = t0 + (idx & (MEL_TF - 1));
            if (t < a.T) out[(size_t)(idx / MEL_TF) * a.T + t] = 0.f;
        }
        return;
    }
    const float *row = a.wav + (size_t)b * a.L;
    // the samples of frame t0 + f, reflected about the row's own ends, as M complex points z[m] = x[2m] + i x[2m + 1] (zeros behind the
    // row's last frame); lane `lane` holds m = lane + 64 r
    auto load_frame = [&](int f, float2 (&z)[R]) {
        const int t = t0 + f, base = t * a.hop - a.pad;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            z[r] = make_float2(0.f, 0.f);
            if (t < Tb) {
                const int j0 = base + 2 * (lane + 64 * r);
                z[r] = make_float2(row[reflect_index(j0, len)], row[reflect_index(j0 + 1, len)]);
            }
        }
    };
    float2 z[R], win[R];
    load_frame(wave, z);
#pragma unroll
    for (int r = 0; r < R; ++r) win[r] = reinterpret_cast<const float2 *>(a.win)[lane + 64 * r];
    for (int i = tid; i < M; i += 64 * MEL_WAVES) tw[i] = a.twm[i];
    for (int i = tid; i < a.kmax; i += 64 * MEL_WAVES) twn[i] = a.twn[i];
    for (int i = tid; i < a.num_mels; i += 64 * MEL_WAVES) rows[i] = a.rows[i];
    for (int i = tid; i < a.nw; i += 64 * MEL_WAVES) wts[i] = a.wts[i];
    lds_barrier();

    // the lane's twiddles of every radix-4 pass, the same for every frame: registers, not LDS reads
    constexpr int NP = (LOGN - 1) / 2, RB = (Q + 63) / 64;
    float2 twr[NP][RB][3];
    {
        int s = 1;
#pragma unroll
        for (int pi = 0; pi < NP; ++pi, s <<= 2)
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int i = (lane + 64 * r) & (Q - 1), ps = i - (i & (s - 1));
                twr[pi][r][0] = tw[ps]; twr[pi][r][1] = tw[2 * ps]; twr[pi][r][2] = tw[3 * ps];
            }
    }
    float2 *A = bufs + wave * 2 * M, *Bf = A + M;
#pragma unroll 1
    for (int f = wave; f < MEL_TF; f += MEL_WAVES) {
#pragma unroll
        for (int r = 0; r < R; ++r) A[fft_at(lane + 64 * r)] = make_float2(z[r].x * win[r].x, z[r].y * win[r].y);
        if (f + MEL_WAVES < MEL_TF) load_frame(f + MEL_WAVES, z);        // the next frame's samples travel while this one is transformed
        wave_lds_sync();
        float2 *x = A, *y = Bf;
        stockham_fft<LOGN>(x, y, [&](int pass, int r, int, int m) { return twr[pass][r][m - 1]; }, lane);
        // ---- real spectrum from the packed transform, magnitude; bins [kmax, kmax + 3) are the zero pad of the last row's chunk
        float *mg = mag + f * a.kstride;
        for (int k = lane; k < a.kmax + 3; k += 64) {
            float v = 0.f;
            if (k < a.kmax) v = mel_magnitude(mel_bin(x[fft_at(k & (M - 1))], x[fft_at((M - k) & (M - 1))], twn[k]));        // X[k] = E + W^k O
            mg[k] = v;
        }
        wave_lds_sync();                  // the next frame overwrites this wave's buffers
    }
    lds_barrier();                        // the projection reads every wave's magnitudes
    // ---- mel projection, clipped log, store with lanes along the frame axis
    for (int idx = tid; idx < a.num_mels * MEL_TF; idx += 64 * MEL_WAVES) {
        const int f = idx & (MEL_TF - 1), i = idx / MEL_TF, t = t0 + f;
        const int4 rw = rows[i];
        const float *mg = mag + f * a.kstride + rw.x;
        const float acc = mel_project(mg, reinterpret_cast<const float4 *>(wts + rw.z), rw.y);
        // the log in float64, rounded once: the AMDGPU expansion of logf (v_log_f32 times ln 2) is two float32 ulps off at -11.5, where
        // the clipped cells of silence sit
        if (t < a.T) out[(size_t)i * a.T + t] = t < Tb ? (float)log((double)fmaxf(acc, 1e-5f)) : 0.f;
    }
}

}  // namespace gtts

using namespace gtts;

namespace {

template <int LOGN>
hipError_t mel_launch(const MelArgs &a, size_t smem, hipStream_t st) {
    const hipError_t e = raise_dyn_lds<&mel_kernel<LOGN>>(smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mel_kernel<LOGN>, dim3((unsigned)((a.T + MEL_TF - 1) / MEL_TF), (unsigned)a.B), dim3(64 * MEL_WAVES), smem, st, a);
    return hipGetLastError();
}

}  // namespace

extern "C" int gtts_mel_create(const gtts_mel_cfg *cfg, gtts_mel **out) {
    if (!cfg || !out) return fail(GTTS_E_NULL, "gtts_mel_create: null argument");
    const gtts_mel_cfg c = *cfg;
    int logn = 0;
    while ((1 << logn) < c.n_fft) ++logn;
    if (c.n_fft < 256 || c.n_fft > 2048 || (1 << logn) != c.n_fft)
        return fail(GTTS_E_CONFIG, "mel: n_fft must be a power of two from 256 to 2048 (got %d)", c.n_fft);
    if (c.win_size < 1 || c.win_size > c.n_fft) return fail(GTTS_E_CONFIG, "mel: win_size must lie in [1, n_fft] (got %d)", c.win_size);
    if (c.hop_size < 1 || c.hop_size > c.n_fft || (c.n_fft - c.hop_size) % 2 != 0)
        return fail(GTTS_E_CONFIG, "mel: hop_size must lie in [1, n_fft] with n_fft - hop_size even (got %d)", c.hop_size);
    if (c.num_mels < 1 || c.num_mels > 128) return fail(GTTS_E_CONFIG, "mel: num_mels must lie in [1, 128] (got %d)", c.num_mels);
    if (c.sampling_rate < 1 || !(c.fmin >= 0.0) || !(c.fmax > c.fmin) || !(c.fmax <= 0.5 * c.sampling_rate))
        return fail(GTTS_E_CONFIG, "mel: need 0 <= fmin < fmax <= sampling_rate / 2 (got %g, %g, %d)", c.fmin, c.fmax, c.sampling_rate);
    gtts_mel *m = new gtts_mel();
    m->cfg = c;
    m->logn = logn;
    m->pad = (c.n_fft - c.hop_size) / 2;
    const int N = c.n_fft, M = N / 2, nb = M + 1;
    slaney_filterbank(c.sampling_rate, c.n_fft, c.num_mels, c.fmin, c.fmax, m->fb);
    // rows: support [k0, k1) of every filter, its weights padded with zeros to whole chunks of four (an empty filter: no chunk, the
    // cell is log(1e-5))
    std::vector<int> rows;
    std::vector<float> wts;
    m->kmax = filter_supports(m->fb, c.num_mels, nb, 4, rows, wts);
    if (m->kmax < 1) m->kmax = 1;
    m->nw = (int)wts.size();
    m->kstride = (m->kmax + 3) | 1;       // every row's last chunk stays inside its frame's magnitudes; odd: frames on different banks
    m->off_win = 0;
    m->off_twm = align256((size_t)N * 4);
    m->off_twn = m->off_twm + align256((size_t)M * 8);
    m->off_rows = m->off_twn + align256((size_t)nb * 8);
    m->off_wts = m->off_rows + align256(rows.size() * 4);
    // the backward's transposed table: the rows that touch bin k are a contiguous row range, as every row's support is a bin range
    std::vector<int> cols(4 * (size_t)m->kmax, 0);
    std::vector<float> wtt;
    for (int k = 0; k < m->kmax; ++k) {
        int i0 = c.num_mels, i1 = 0;
        for (int i = 0; i < c.num_mels; ++i)
            if (m->fb[(size_t)i * nb + k] != 0.f) { i0 = i < i0 ? i : i0; i1 = i + 1; }
        if (i1 == 0) i0 = 0;
        cols[4 * k] = i0; cols[4 * k + 1] = i1 - i0; cols[4 * k + 2] = (int)wtt.size();
        for (int i = i0; i < i1; ++i) wtt.push_back(m->fb[(size_t)i * nb + k]);
    }
    if (wtt.empty()) wtt.push_back(0.f);
    m->off_cols = m->off_wts + align256(wts.size() * 4);
    m->off_wtt = m->off_cols + align256(cols.size() * 4);
    m->image.assign(m->off_wtt + align256(wtt.size() * 4), 0);
    memcpy(m->image.data() + m->off_cols, cols.data(), cols.size() * 4);
    memcpy(m->image.data() + m->off_wtt, wtt.data(), wtt.size() * 4);
    m->smem_bwd = mel_backward_lds(M, m->kstride, c.num_mels, m->nw);
    float *win = reinterpret_cast<float *>(m->image.data() + m->off_win);
    float *twm = reinterpret_cast<float *>(m->image.data() + m->off_twm), *twn = reinterpret_cast<float *>(m->image.data() + m->off_twn);
    const int left = (N - c.win_size) / 2;
    for (int n = 0; n < c.win_size; ++n) win[left + n] = (float)hann_periodic(n, c.win_size);
    fill_twiddles(twm, M, M);
    fill_twiddles(twn, nb, N);
    memcpy(m->image.data() + m->off_rows, rows.data(), rows.size() * 4);
    memcpy(m->image.data() + m->off_wts, wts.data(), wts.size() * 4);
    m->smem = (size_t)M * 8 + (size_t)(M + 2) * 8 + (size_t)MEL_WAVES * 2 * M * 8 + (size_t)((MEL_TF * m->kstride + 3) & ~3) * 4 + (size_t)c.num_mels * 16 + (size_t)m->nw * 4;
    if (m->smem > 160 * 1024) {
        delete m;
        return fail(GTTS_E_CONFIG, "mel: the configuration needs more than 160 KB of LDS");
    }
    *out = m;
    return GTTS_OK;
}

extern "C" void gtts_mel_destroy(gtts_mel *m) { delete m; }

extern "C" int gtts_mel_frames(const gtts_mel *m, int L) {
    if (!m) return fail(GTTS_E_NULL, "gtts_mel_frames: null handle");
    if (L <= m->pad) return fail(GTTS_E_SHAPE, "mel: %d samples cannot be reflect-padded by %d (needs L > pad)", L, m->pad);
    if (L > 0x7fffffff - 2 * m->pad) return fail(GTTS_E_SHAPE, "mel: %d samples are too many for 32-bit sample indices", L);
    if (L + 2 * m->pad < m->cfg.n_fft) return fail(GTTS_E_SHAPE, "mel: %d samples hold no whole frame of %d", L, m->cfg.n_fft);
    return mel_frames_of(L, m->cfg.n_fft, m->cfg.hop_size, m->pad);
}

extern "C" size_t gtts_mel_packed_bytes(const gtts_mel *m) { return m ? m->image.size() : 0; }

extern "C" int gtts_mel_pack(const gtts_mel *m, void *packed, gtts_stream_t stream) {
    if (!m || !packed) return fail(GTTS_E_NULL, "gtts_mel_pack: null argument");
    GTTS_HIPCHK(hipMemcpyAsync(packed, m->image.data(), m->image.size(), hipMemcpyHostToDevice, (hipStream_t)stream));
    return GTTS_OK;
}

extern "C" int gtts_mel_filterbank(const gtts_mel *m, float *host_out) {
    if (!m || !host_out) return fail(GTTS_E_NULL, "gtts_mel_filterbank: null argument");
    memcpy(host_out, m->fb.data(), m->fb.size() * 4);
    return GTTS_OK;
}

extern "C" int gtts_mel_forward(const gtts_mel *m, const void *packed, const float *wav, const int *lengths, float *out, int B, int L,
                                gtts_stream_t stream) {
    if (!m || !packed || !wav || !out) return fail(GTTS_E_NULL, "gtts_mel_forward: null argument");
    if (B <= 0 || B > 65535) return fail(GTTS_E_SHAPE, "gtts_mel_forward: B must lie in [1, 65535] (got %d)", B);
    const int T = gtts_mel_frames(m, L);
    if (T < 0) return T;
    const unsigned char *blob = static_cast<const unsigned char *>(packed);
    MelArgs a;
    a.wav = wav; a.lengths = lengths; a.out = out;
    a.win = reinterpret_cast<const float *>(blob + m->off_win);
    a.twm = reinterpret_cast<const float2 *>(blob + m->off_twm);
    a.twn = reinterpret_cast<const float2 *>(blob + m->off_twn);
    a.rows = reinterpret_cast<const int4 *>(blob + m->off_rows);
    a.wts = reinterpret_cast<const float *>(blob + m->off_wts);
    a.B = B; a.L = L; a.T = T; a.hop = m->cfg.hop_size; a.pad = m->pad; a.num_mels = m->cfg.num_mels;
    a.kmax = m->kmax; a.kstride = m->kstride; a.nw = m->nw;
    hipStream_t st = (hipStream_t)stream;
    switch (m->logn) {
        case 8: GTTS_HIPCHK(mel_launch<8>(a, m->smem, st)); break;
        case 9: GTTS_HIPCHK(mel_launch<9>(a, m->smem, st)); break;
        case 10: GTTS_HIPCHK(mel_launch<10>(a, m->smem, st)); break;
        default: GTTS_HIPCHK(mel_launch<11>(a, m->smem, st)); break;
    }
    return GTTS_OK;
}
