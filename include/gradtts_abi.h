/*
 * gradtts_abi.h -- C ABI of libgradtts_gfx950.so, the MI355X-native Grad-TTS / DiffVC decoder sampling path.
 *
 * This is the drop-in boundary.  The reference has no FFI of its own: its hot path is
 * Python calling torch ops.  Each entry point below therefore names the reference *Python* symbol it
 * replaces; the Python host (the modules under speech-backbones_amd/model/) keeps that symbol's signature and calls these
 * functions through ctypes.  INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch types.  All tensors are fp32, contiguous, row-major, in the
 *     reference's own layouts ([B,80,T] mels, [B,1,T] masks flattened to [B,T], NCHW inside).
 *   - the CALLER owns every device buffer (inputs, outputs, packed weights, workspace); the library never
 *     allocates device memory and keeps no device pointer after a call returns.  Workspace, scratch, saved-state and
 *     output buffers (a packed-weight blob before its pack call included) may hold ANY bytes on entry: no result depends on
 *     what a call did not write itself (tests/test_gpu_fresh_memory.py).
 *   - every call enqueues on the given hipStream_t and returns without synchronising (two documented exceptions, both off the
 *     sampling path: gtts_pack_weights of a GTTS_PREC_F16F8 plan and gtts_workspace_status).  The sampler may fan sub-batches
 *     out onto side streams, but only onto streams the CALLER registered with gtts_plan_set_streams (they are forked
 *     from and joined back into the call's stream inside the call, also on error paths).
 *   - a plan is host-side metadata.  Query functions take `const gtts_plan *` and touch nothing; the enqueueing
 *     functions take `gtts_plan *` and serialise on a mutex inside the plan for the duration of the host-side enqueue,
 *     so a plan may be shared by host threads as long as every call brings its own workspace.
 *   - no environment variable changes results; diagnostics (op skipping, phase traces, timing ablations) exist only in
 *     -DGTTS_DIAG builds, never in the product library.
 *   - every function returns 0 on success or a negative GTTS_E_* code; gtts_last_error() gives the text
 *     (thread-local).  No C++ exception crosses the boundary.
 *   - T (frames) must be a multiple of 4 (Grad-TTS/model/utils.py:13-17 fix_len_compatibility), n_feats a
 *     multiple of 4.
 */
#ifndef GRADTTS_ABI_H
#define GRADTTS_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GTTS_ABI_VERSION 7

enum {
    GTTS_OK = 0,
    GTTS_E_NULL = -1,        /* required pointer is NULL                                  */
    GTTS_E_SHAPE = -2,       /* bad B/T/F (T % 4 != 0, non-positive sizes, ...)           */
    GTTS_E_CONFIG = -3,      /* unsupported model configuration                           */
    GTTS_E_HIP = -4,         /* HIP launch / runtime error (text in gtts_last_error)      */
    GTTS_E_PARAMS = -5,      /* parameter list does not match the plan's state_dict layout */
    GTTS_E_WORKSPACE = -6,   /* workspace too small                                       */
    GTTS_E_RANGE = -7        /* ABI 6: a value lies outside the range the plan's precision represents (GTTS_PREC_F16F8 weights) */
};

/* precision of the dense contractions (3x3 / 1x1 / transposed convs, attention products) */
enum {
    GTTS_PREC_BF16X3 = 0,    /* split-bf16 (hi/lo, 3 MFMAs, fp32 accumulate): fp32-grade accuracy                 */
    GTTS_PREC_BF16 = 1,      /* single bf16 MFMA, fp32 accumulate, fp32 activation storage                   */
    GTTS_PREC_BF16_STORE = 2,/* BASELINE.json config 3 as written: single bf16 MFMA, fp32 accumulate, and every
                                activation tensor of the U-Net stored as bf16 (weights are bf16 already); GroupNorm
                                statistics come from the fp32 accumulators before rounding.  Grad-TTS plans only. */
    GTTS_PREC_F16F8 = 3      /* ABI 5.  fp32-grade like BF16X3 (~2^-17 per product), two MFMA pass-equivalents instead of three
                                on the 3x3 Block convolutions and the Upsample transposed convolutions: x = fp16 hi + residual; hi*hi on the fp16 MFMA, both cross terms
                                (w * x_lo + w_lo * x, operands rounded to fp8 e4m3) in ONE fp8 MFMA per 32 channels.  Every other
                                contraction of the plan (1x1, Downsample, attention, the 2-channel first layer) stays BF16X3.
                                RANGE CONTRACT (ABI 6, enforced): the weights of those layers must satisfy |w| < 63.97 (w 2^10
                                in fp16) -- gtts_pack_weights checks every such weight on the device and returns GTTS_E_RANGE
                                naming a layer (nothing is ever packed as inf); an activation with |x| >= 1024 keeps an
                                fp16-grade cross term only (its fp8 operand saturates; beyond 65504 the fp16 half overflows) --
                                the staging kernels record every such event and the maximum |x| in the first 16 bytes of the
                                caller's workspace, read with gtts_workspace_status.
                                cfg.conv_ws selects the kernel (persistent / uniform waves) AND which layers take the split: the
                                64-channel layers only with conv_ws = 1.  A packed blob is valid for the plan it was packed for. */
};

typedef void *gtts_stream_t; /* hipStream_t */

/* Mirrors GradLogPEstimator2d.__init__ (Grad-TTS/model/diffusion.py:129-130) plus Diffusion's betas
 * (diffusion.py:228-230). */
typedef struct gtts_unet_cfg {
    int dim;             /* dec_dim, 64                                      */
    int n_feats;         /* 80                                               */
    int n_spks;          /* 1 -> 2 input channels; >1 -> 3 + spk_mlp         */
    int spk_emb_dim;     /* 64                                               */
    int groups;          /* GroupNorm groups, 8                              */
    float pe_scale;      /* 1000                                             */
    float beta_min;      /* 0.05                                             */
    float beta_max;      /* 20.0                                             */
    int precision;       /* GTTS_PREC_*                                      */
    int keep_intermediates; /* 1: every op output gets its own workspace slot (tests / debugging)       */
    /* ---- DiffVC decoder (DiffVC/model/diffusion.py:17-59): arch = 1, dim = dim_base (256), pe_scale 1000 */
    int arch;            /* 0: Grad-TTS GradLogPEstimator2d, 1: DiffVC GradLogPEstimator                 */
    int dim_cond;        /* 128: condition channels appended to [mean, x] (130 input channels)          */
    int use_ref_t;       /* 1: RefBlock on the diffused reference mel feeds the condition                */
    int c_dim;           /* 256: speaker-embedding width                                                 */
    double vc_beta_min;  /* DiffVC schedule scalars are Python doubles in the reference (diffusion.py:120-149) */
    double vc_beta_max;
    /* ---- ABI 3: which kernel runs the Block 3x3 convolutions of 128-channel-and-wider layers in GTTS_PREC_BF16X3 / F16F8 ---- */
    int conv_ws;         /* 0: uniform-wave kernel (conv_mfma.hip; overlaps with other streams' kernels: best with three
                            sub-batch streams in BF16X3 on the Grad-TTS dim-64 network).  1: persistent wave-specialised kernel
                            (conv_ws.hip; a higher MFMA rate per launch, but it fills every CU's registers: best where these
                            convolutions dominate -- the DiffVC dim-256 decoder -- and in GTTS_PREC_F16F8, where it also runs the
                            64-channel layers, unsplit).  Either way results do not depend on the batch split; the two modes
                            agree to fp32 rounding of the GroupNorm statistics. */
} gtts_unet_cfg;

typedef struct gtts_plan gtts_plan;   /* host-side metadata only */

int gtts_abi_version(void);
const char *gtts_last_error(void);

/* ---- plan ------------------------------------------------------------------------------------------ */
int gtts_plan_create(const gtts_unet_cfg *cfg, gtts_plan **out);
void gtts_plan_destroy(gtts_plan *plan);

/* state_dict layout the plan expects, in the reference's registration order:
 * name (relative to `estimator.`), rank and dims of parameter i; count via gtts_plan_num_params. */
int gtts_plan_num_params(const gtts_plan *plan);
int gtts_plan_param_info(const gtts_plan *plan, int i, const char **name, int *rank, int dims[4]);

size_t gtts_packed_weight_bytes(const gtts_plan *plan);
/* Workspace for gtts_estimator_forward / gtts_reverse_diffusion at (B,T); depends on the number of registered side
 * streams (each sub-batch works in its own slice), so query it AFTER gtts_plan_set_streams. */
size_t gtts_workspace_bytes(const gtts_plan *plan, int B, int T);

/* Register n in {0, 2, 3, 4} caller-owned side streams (hipStream_t) on which gtts_reverse_diffusion runs sub-batches
 * of the utterance batch side by side (bit-identical results; utterances are independent).  n = 0 (default): everything
 * runs on the stream passed to the call.  The streams must outlive the plan or be unregistered (n = 0) first. */
int gtts_plan_set_streams(gtts_plan *plan, const gtts_stream_t *streams, int n);

/* on != 0: gtts_reverse_diffusion captures the launches of a call into a hipGraph the first time it sees an argument
 * tuple (all pointers, shapes and the step range are part of the key) and replays it with one hipGraphLaunch on later
 * calls with the same tuple -- for the launch-bound small-batch regime (B = 1 inference, Grad-TTS/inference.py:62-76).
 * Keep the buffers alive and at the same addresses to hit the cache (at most 8 graphs are kept, LRU).  on == 0 drops
 * the cached graphs.  Results are identical to the eager path (same kernels, same order). */
int gtts_plan_set_graph(gtts_plan *plan, int on);

/* Re-layout the estimator parameters (device fp32 pointers, in gtts_plan_param_info order) into the packed
 * blob the kernels read (bf16 hi/lo MFMA fragment order for conv weights, fp32 for the rest).
 * `freq` = the 32 (dim/2) sinusoidal frequencies exp(-k ln(1e4)/(dim/2-1)) as fp32 device values computed by
 * the host exactly as SinusoidalPosEmb does (diffusion.py:121-122).
 * GTTS_PREC_F16F8 plans (ABI 6): the packer range-checks the 3x3 Block-convolution weights on the device and this call then
 * SYNCHRONISES `stream` to read the verdict: GTTS_E_RANGE (text names the count, max |w| and a layer) when a weight does not fit
 * the format; the blob must then not be used -- pack the model with a GTTS_PREC_BF16X3 plan instead. */
int gtts_pack_weights(const gtts_plan *plan, const void *const *param_ptrs, int n_params, const float *freq,
                      void *packed, gtts_stream_t stream);

/* ABI 6.  Activation range record of the last gtts_estimator_forward / gtts_reverse_diffusion (or gtts_vc_*) call that used
 * `workspace`: *n_events = number of staging lanes x launches that split an activation with |x| >= 1024 (GTTS_PREC_F16F8 plans
 * only), plus -- in every precision -- (samples x Block convolutions) whose GroupNorm statistics came out non-finite;
 * *max_abs = the largest |x| seen (inf for a non-finite one; 0 when n_events == 0).  Sticky over the step ranges of one
 * sampling run (reset where step_begin == 0, and by every estimator call).  This query -- and gtts_pack_weights of an F16F8 plan --
 * are the only calls of the ABI that SYNCHRONISE `stream`; do not call them inside a stream capture. */
int gtts_workspace_status(const void *workspace, unsigned *n_events, float *max_abs, gtts_stream_t stream);

/* ---- GradLogPEstimator2d.forward(x, mask, mu, t, spk)  diffusion.py:174-216 -------------------------- */
/* x, mu, out [B,F,T]; mask [B,T]; t [B]; spk [B,spk_emb_dim] (already embedded) or NULL. */
int gtts_estimator_forward(gtts_plan *plan, const void *packed, const float *x, const float *mask,
                           const float *mu, const float *t, const float *spk, float *out, void *workspace,
                           size_t workspace_bytes, int B, int T, gtts_stream_t stream);

/* ---- one update of Diffusion.reverse_diffusion  diffusion.py:264-274 --------------------------------- */
/* xt is updated IN PLACE.  noise == NULL: ODE branch; else SDE branch with the pre-drawn N(0,1) tensor. */
int gtts_euler_step(float *xt, const float *mu, const float *est, const float *mask, const float *noise,
                    float beta_t, float h, int B, int F, int T, gtts_stream_t stream);

/* ---- Diffusion.reverse_diffusion / forward  diffusion.py:254-279 (whole N-step loop) ------------------ */
/* z, mu, out [B,F,T]; mask [B,T]; spk nullable.  Runs steps [step_begin, step_end) of the n_timesteps-step schedule:
 * step_begin == 0 first sets out = z * mask, later ranges continue in place on `out`, so a host can draw the SDE noise
 * in bounded chunks.  noise nullable [step_end - step_begin, B,F,T] (stoc=True <=> noise != NULL). */
int gtts_reverse_diffusion(gtts_plan *plan, const void *packed, const float *z, const float *mask,
                           const float *mu, const float *spk, const float *noise, float *out, void *workspace,
                           size_t workspace_bytes, int B, int T, int n_timesteps, int step_begin, int step_end,
                           gtts_stream_t stream);

/* ---- DiffVC: GradLogPEstimator.forward(x, x_mask, mean, ref, ref_mask, c, t)  DiffVC/model/diffusion.py:61-106 -- */
/* x, mean, out [B,F,T]; x_mask [B,T]; xt_ref [B,1,F,T_ref] (the diffused reference, diffusion.py:173-176);
 * ref_mask [B,T_ref]; c [B,c_dim]; t [B].  T % 4 == 0; T_ref is free. */
size_t gtts_vc_workspace_bytes(const gtts_plan *plan, int B, int T, int T_ref);
int gtts_vc_estimator_forward(gtts_plan *plan, const void *packed, const float *x, const float *x_mask,
                              const float *mean, const float *xt_ref, const float *ref_mask, const float *c, const float *t,
                              float *out, void *workspace, size_t workspace_bytes, int B, int T, int T_ref,
                              gtts_stream_t stream);
/* ---- DiffVC: Diffusion.reverse_diffusion / forward  DiffVC/model/diffusion.py:164-205 ------------------------ */
/* mode 0 'pf', 1 'em', 2 'ml'; steps [step_begin, step_end) as in gtts_reverse_diffusion; noise
 * [step_end - step_begin, B,F,T] pre-drawn N(0,1) (required for em / ml, ignored for pf); ref, mean_ref [B,F,T_ref].
 * The schedule scalars (beta, gamma, mu, nu, sigma, kappa, omega) are host doubles. */
int gtts_vc_reverse_diffusion(gtts_plan *plan, const void *packed, const float *z, const float *mask,
                              const float *mean, const float *ref, const float *ref_mask, const float *mean_ref,
                              const float *c, const float *noise, float *out, void *workspace, size_t workspace_bytes, int B,
                              int T, int T_ref, int n_timesteps, int mode, int step_begin, int step_end,
                              gtts_stream_t stream);

/* ---- monotonic_align.maximum_path  monotonic_align/core.pyx:9-45 + __init__.py:8-23 ------------------- */
/* value [b,tx,ty] fp32 (NOT modified), mask [b,tx,ty] fp32 or NULL, t_x / t_y [b] int32 device arrays,
 * path [b,tx,ty] int32 (written: 0/1), scratch >= gtts_mas_scratch_bytes(b,tx,ty) device bytes.  t_x[i] > t_y[i] (an empty band in
 * core.pyx:18) follows the reference too: its backtrack over the untouched values. */
size_t gtts_mas_scratch_bytes(int b, int tx, int ty);
int gtts_mas_maximum_path(const float *value, const float *mask, const int *t_x, const int *t_y, int *path,
                          void *scratch, int b, int tx, int ty, gtts_stream_t stream);

/* CPU twin (host pointers, no stream): the reference's maximum_path accepts tensors on any device and runs its Cython
 * kernel on the host (__init__.py:8-23); bit-identical to the GPU kernel and to core.pyx. */
int gtts_mas_maximum_path_cpu(const float *value, const float *mask, const int *t_x, const int *t_y, int *path, int b,
                              int tx, int ty);

/* ---- multi-GPU: the single collective -- RCCL broadcast of the packed weight blob from `root` over xGMI.
 * comm = the caller's ncclComm_t.  RCCL is resolved from the running process at call time (no link-time dependency). */
int gtts_bcast_weights(void *packed, size_t bytes, int root, void *comm, gtts_stream_t stream);

/* ---- pre-decoder glue of GradTTS.forward: generate_path + mu_y = attn^T . mu_x + z  (tts.py:84-94, utils.py:26-39) -
 * duration [B,t_x] fp32 (= w_ceil incl. length_scale), x_mask [B,t_x] fp32, y_lengths [B] int32 (device),
 * mu_x [B,F,t_x]; noise [B,F,T] or NULL, temperature; outputs attn [B,t_x,T], mu_y [B,F,T], z [B,F,T] (z may be NULL;
 * noise NULL gives z = mu_y).  Bit-identical to the reference's CPU path (sequential fp32 cumsum, float compares). */
int gtts_expand_alignment(const float *duration, const float *x_mask, const int *y_lengths, const float *mu_x,
                          const float *noise, float temperature, float *attn, float *mu_y, float *z, int B, int F,
                          int t_x, int T, gtts_stream_t stream);

/* ---- MAS score matrix of GradTTS.compute_loss  (tts.py:130-139): log N(y_j; mu_x_i, I) for every (token i, frame j) --
 * mu_x [B,F,t_x], y [B,F,T] -> log_prior [B,t_x,T] (fp32, feeds gtts_mas_maximum_path without leaving the device).
 * Evaluated as -0.5 sum_f (y - mu)^2 - 0.5 F log(2 pi): equal to the reference's three-matmul form up to fp32 rounding. */
int gtts_log_prior(const float *mu_x, const float *y, float *log_prior, int B, int F, int t_x, int T, gtts_stream_t stream);

/* ---- HiFi-GAN generator: mel -> waveform, the step after the sampling path (Grad-TTS/inference.py:81;
 * Grad-TTS/hifi-gan/models.py:77-128, configuration Grad-TTS/checkpts/hifigan-config.json) ------------------------------ */
typedef struct gtts_voc_cfg {
    int n_mels;                       /* 80                                                            */
    int upsample_initial_channel;     /* 512                                                           */
    int n_ups;                        /* len(upsample_rates), <= 8                                     */
    int upsample_rates[8];            /* 8,8,2,2      (powers of two)                                  */
    int upsample_kernel_sizes[8];     /* 16,16,4,4    (= 2 * rate)                                     */
    int n_kernels;                    /* len(resblock_kernel_sizes), <= 8                              */
    int resblock_kernel_sizes[8];     /* 3,7,11       (odd, <= 11)                                     */
    int resblock_dilations[8][3];     /* 1,3,5 each   (ResBlock2 uses the first two)                   */
    int resblock_type;                /* 1: ResBlock1 (models.py:13-50), 2: ResBlock2 (:53-74)         */
} gtts_voc_cfg;
typedef struct gtts_voc gtts_voc;     /* host-side metadata only */
int gtts_voc_create(const gtts_voc_cfg *cfg, gtts_voc **out);
void gtts_voc_destroy(gtts_voc *voc);
/* parameter i of the layout the packer expects: `<module path>.weight` / `.bias` with weight normalisation already
 * folded (Generator.remove_weight_norm, models.py:122-128); Conv1d weights [cout][cin][k], ConvTranspose1d [cin][cout][k] */
int gtts_voc_num_params(const gtts_voc *voc);
int gtts_voc_param_info(const gtts_voc *voc, int i, const char **name, int *rank, int dims[4]);
size_t gtts_voc_packed_bytes(const gtts_voc *voc);
int gtts_voc_pack(const gtts_voc *voc, const void *const *param_ptrs, int n_params, void *packed, gtts_stream_t stream);
size_t gtts_voc_workspace_bytes(const gtts_voc *voc, int B, int T);
int gtts_voc_hop(const gtts_voc *voc);          /* output samples per mel frame (product of the rates: 256) */
/* Generator.forward: mel [B, n_mels, T] fp32 -> wav [B, 1, T * hop] fp32 in (-1, 1). */
int gtts_voc_forward(const gtts_voc *voc, const void *packed, const float *mel, float *wav, void *workspace,
                     size_t workspace_bytes, int B, int T, gtts_stream_t stream);

/* ---- encoders either side of the sampling path: Grad-TTS TextEncoder (Grad-TTS/model/text_encoder.py:281-326) and DiffVC
 * MelEncoder (DiffVC/model/encoder.py:257-284); inference only (dropout = identity) ------------------------------------- */
typedef struct gtts_enc_cfg {
    int mode;                 /* 0: TextEncoder (ids -> mu, logw), 1: MelEncoder (mel -> mel)                         */
    int n_vocab;              /* 149 (TextEncoder)                                                                    */
    int n_feats;              /* 80                                                                                   */
    int channels;             /* n_enc_channels 192                                                                   */
    int filter_channels;      /* 768                                                                                  */
    int filter_channels_dp;   /* 256 (TextEncoder's DurationPredictor)                                                */
    int n_heads;              /* 2                                                                                    */
    int n_layers;             /* 6                                                                                    */
    int kernel_size;          /* 3 (FFN / DurationPredictor convolutions; odd)                                        */
    int window_size;          /* 4 (relative-position window; 0: none)                                                */
} gtts_enc_cfg;
typedef struct gtts_enc gtts_enc;
int gtts_enc_create(const gtts_enc_cfg *cfg, gtts_enc **out);
void gtts_enc_destroy(gtts_enc *enc);
/* parameters in the reference module's registration order, names relative to the encoder module (e.g. `emb.weight`,
 * `prenet.conv_layers.0.weight`, `encoder.attn_layers.0.emb_rel_k`, `proj_w.norm_1.gamma`) */
int gtts_enc_num_params(const gtts_enc *enc);
int gtts_enc_param_info(const gtts_enc *enc, int i, const char **name, int *rank, int dims[4]);
size_t gtts_enc_packed_bytes(const gtts_enc *enc);
int gtts_enc_pack(const gtts_enc *enc, const void *const *param_ptrs, int n_params, void *packed, gtts_stream_t stream);
size_t gtts_enc_workspace_bytes(const gtts_enc *enc, int B, int L);
/* Which attention kernel gtts_enc_forward runs at sequence length L: 16 (16 queries per workgroup, lanes along the keys: needs
 * channels / n_heads % 4 == 0, window_size <= 7 and (16 * channels / n_heads + 16 * roundup(L, 64) + 512) * 4 <= 160 KB of LDS),
 * 8 (8 queries per workgroup: (8 * channels / n_heads + 8 * L) * 4 <= 160 KB), or 0: gtts_enc_forward refuses L with GTTS_E_SHAPE
 * (also for a null encoder or L <= 0).  The defaults (192 channels, 2 heads, window 4): 16 up to L = 2432, 8 up to 5024. */
int gtts_enc_attention_path(const gtts_enc *enc, int L);
/* mode 0: ids [B,L] int64 (device), x_mask [B,L] fp32 -> mu [B,n_feats,L], logw [B,1,L];  mel is ignored.
 * mode 1: mel [B,n_feats,L], x_mask -> mu [B,n_feats,L] (the encoded mel); ids / logw are ignored. */
int gtts_enc_forward(const gtts_enc *enc, const void *packed, const long long *ids, const float *mel, const float *x_mask,
                     float *mu, float *logw, void *workspace, size_t workspace_bytes, int B, int L, gtts_stream_t stream);
/* ---- ABI 6 (additive): the encoders' two fp32 VALU ops as calls of their own -- the entries their per-op tests drive;
 * gtts_enc_forward reaches its kernels through the same two launch functions.  All tensors fp32, contiguous, t fastest.
 *
 * gtts_enc_layernorm: LayerNorm over the channel axis per position (text_encoder.py:12-27: biased variance, two passes):
 *   out[b][c][t] = relu_out?( (v - mean_c v) * rsqrt(var_c v + eps) * gamma[c] + beta[c] ) * out_mask[b][t],
 *   v = relu_in?(a[b][c][t]) * a_mask[b][t] + bres[b][c][t].   a, bres, out [B][C][L]; gamma, beta [C]; a_mask, out_mask [B][L];
 *   bres, a_mask and out_mask may be NULL (no residual / no mask); out must not overlap an input.
 *   GTTS_E_NULL: a, gamma, beta or out NULL; GTTS_E_SHAPE: B, C or L < 1 or B > 65535; GTTS_E_CONFIG: eps <= 0.
 *
 * gtts_enc_attention: MultiHeadAttention.attention (text_encoder.py:145-175), self-attention with a relative window:
 *   q, k, v, out [B][C][L] (head h = channels [h dk, (h + 1) dk), dk = C / n_heads), mask [B][L] (0 / 1: a score whose query or key is
 *   masked is -1e4 before the softmax), emb_rel_k, emb_rel_v [2 window + 1][dk] shared by all heads.  window 0: no relative terms,
 *   the two embedding pointers are not read and may be NULL.  path 0: the kernel gtts_enc_forward would run
 *   (gtts_enc_attention_path_for); 16 / 8: that kernel.  Refused on the host before the device is touched:
 *   GTTS_E_NULL (a required pointer), GTTS_E_SHAPE (B or L < 1, B or n_heads > 65535, L beyond the 160 KB of LDS of the kernel asked
 *   for -- or of both under path 0), GTTS_E_CONFIG (C % n_heads, window < 0, a path other than 0 / 8 / 16, path 16 with dk % 4 != 0 or
 *   window > 7). */
int gtts_enc_layernorm(const float *a, const float *bres, const float *gamma, const float *beta, const float *a_mask,
                       const float *out_mask, float *out, int B, int C, int L, float eps, int relu_in, int relu_out, gtts_stream_t stream);
int gtts_enc_attention(const float *q, const float *k, const float *v, const float *mask, const float *emb_rel_k,
                       const float *emb_rel_v, float *out, int B, int C, int L, int n_heads, int window, int path, gtts_stream_t stream);
/* host only, no encoder handle: gtts_enc_attention_path for an encoder of these channels, heads and window at length L (0 also for
 * channels, n_heads < 1, channels % n_heads != 0 or window < 0) */
int gtts_enc_attention_path_for(int channels, int n_heads, int window, int L);

/* ---- ABI 7 (additive): TRAINING of the same two ops (csrc/enc_train.hip) -- the attention core forward with dropout and its backward,
 * and the backward of gtts_enc_layernorm (whose forward under autograd is gtts_enc_layernorm itself).  All tensors fp32, contiguous,
 * t fastest, on `stream`; nothing L x L is kept between forward and backward, no floating-point atomics: the same inputs give the
 * same bits.  Every refusal below happens on the host before the device is touched.
 *
 * gtts_enc_attention_train_ok (host only): 1 where the three training kernels hold the shape in 160 KB of LDS, else 0 (also for
 *   channels, n_heads < 1, channels % n_heads != 0, window < 0, L < 1).  With dk = channels / n_heads, R = 2 window + 1 (0 without a
 *   window) and LP = roundup(L, 64), in floats:   forward 16 dk + 16 R + 16 LP + 16;   query-tiled backward 16 dk + 16 R + 16 LP + 32;
 *   key-tiled backward 288 dk + 32 R + 2112 (no L).  dk <= 96 with window <= 7: every L <= 2432 (the defaults, dk 96 and window 4: 2432 is the last).
 *
 * gtts_enc_attention_train_forward: gtts_enc_attention's semantics (q, k, v, out [B][C][L], mask [B][L], emb_rel_k / emb_rel_v
 *   [2 window + 1][dk]; window 0: both may be NULL) plus
 *   drop  [B][H][L][L] or NULL: multiplier (0 or 1 / (1 - p)) applied to the probabilities after the softmax;
 *   stat  [B][H][L][2], written: per query row the score maximum and the reciprocal of its exponential sum.
 * gtts_enc_attention_train_backward: dout [B][C][L] -> dq, dk, dv [B][C][L], dek, dev [2 window + 1][dk] (window 0: may be NULL, not
 *   written), from the forward's inputs, `drop` and `stat`;  scratch of gtts_enc_attention_train_scratch_bytes(B, C, L, n_heads, window)
 *   bytes (0 for a refused shape).  A score that was replaced by -1e4 passes no gradient; rows of padded queries still reach dv.
 *   GTTS_E_NULL (a required pointer), GTTS_E_SHAPE (B or L < 1, B or n_heads > 65535, L beyond gtts_enc_attention_train_ok),
 *   GTTS_E_CONFIG (C % n_heads, window < 0, a head width / window no length fits). */
int gtts_enc_attention_train_ok(int channels, int n_heads, int window, int L);
size_t gtts_enc_attention_train_scratch_bytes(int B, int C, int L, int n_heads, int window);
int gtts_enc_attention_train_forward(const float *q, const float *k, const float *v, const float *mask, const float *emb_rel_k,
                                     const float *emb_rel_v, const float *drop, float *out, float *stat, int B, int C, int L, int n_heads,
                                     int window, gtts_stream_t stream);
int gtts_enc_attention_train_backward(const float *q, const float *k, const float *v, const float *mask, const float *emb_rel_k,
                                      const float *emb_rel_v, const float *drop, const float *stat, const float *dout, float *dq, float *dk,
                                      float *dv, float *dek, float *dev, void *scratch, int B, int C, int L, int n_heads, int window,
                                      gtts_stream_t stream);
/* gtts_enc_layernorm_backward: gradients of  out = relu_out?(LN_c(relu_in?(a) * a_mask + bres)) * out_mask  (gtts_enc_layernorm) from
 *   dout [B][C][L]: da [B][C][L], dbres [B][C][L] (written only when bres is given), dgamma, dbeta [C].  Mean and rstd are recomputed from
 *   the inputs in two passes; ReLU' (0) = 0; beta is read only to recompute the sign under relu_out; dgamma / dbeta are per-workgroup
 *   partials (scratch: gtts_enc_layernorm_backward_scratch_floats(B, C, L) floats, 0 for a refused shape) folded in a fixed order.
 *   GTTS_E_NULL: dout, a, gamma, beta, da, dgamma, dbeta or scratch NULL, bres without dbres; GTTS_E_SHAPE: B, C or L < 1 or
 *   B > 65535; GTTS_E_CONFIG: eps <= 0. */
size_t gtts_enc_layernorm_backward_scratch_floats(int B, int C, int L);
int gtts_enc_layernorm_backward(const float *dout, const float *a, const float *bres, const float *gamma, const float *beta,
                                const float *a_mask, const float *out_mask, float *da, float *dbres, float *dgamma, float *dbeta,
                                float *scratch, int B, int C, int L, float eps, int relu_in, int relu_out, gtts_stream_t stream);

/* ---- DiffVC PostNet (DiffVC/model/postnet.py:40-53; the last stage of the "average voice" encoder, vc.py:33-41):
 * x [B,n_feats,T], mask [B,T] -> out [B,n_feats,T].  dim % 64 == 0, 8 GroupNorm groups.  Parameter names are the module's
 * state_dict keys (`init_conv.weight`, `res_block.block1.block.0.weight` [dim,dim,7,7], ...). */
typedef struct gtts_postnet gtts_postnet;
int gtts_postnet_create(int dim, int n_feats, int groups, gtts_postnet **out);
void gtts_postnet_destroy(gtts_postnet *pn);
int gtts_postnet_num_params(const gtts_postnet *pn);
int gtts_postnet_param_info(const gtts_postnet *pn, int i, const char **name, int *rank, int dims[4]);
size_t gtts_postnet_packed_bytes(const gtts_postnet *pn);
int gtts_postnet_pack(const gtts_postnet *pn, const void *const *param_ptrs, int n_params, void *packed, gtts_stream_t stream);
size_t gtts_postnet_workspace_bytes(const gtts_postnet *pn, int B, int T);
int gtts_postnet_forward(const gtts_postnet *pn, const void *packed, const float *x, const float *mask, float *out,
                         void *workspace, size_t workspace_bytes, int B, int T, gtts_stream_t stream);

/* ---- training hot path, first kernels (Grad-TTS/train.py:105-119; Grad-TTS/model/diffusion.py:244-252,281-294) --------
 * The host (model/_train_ops.py) wraps these and the entry points further down in torch.autograd.Function; autograd only
 * sequences them (and adds gradient accumulations). */
/* Diffusion.forward_diffusion: xt = (x0 d + mu (1-d) + z sqrt(1 - e^{-cum})) mask, z_masked = z mask; d = e^{-cum/2},
 * cum = beta_min t + (beta_max - beta_min) t^2 / 2 per sample; x0, mu, z, xt, z_masked [B,F,T], mask [B,T], t [B]. */
int gtts_diffusion_noising(const float *x0, const float *mu, const float *z, const float *mask, const float *t, float beta_min,
                           float beta_max, float *xt, float *z_masked, int B, int F, int T, gtts_stream_t stream);
/* Diffusion.loss_t: r = eps sqrt(1 - e^{-cum}) + z_masked; partials[i] = sum of r^2 over 256-element blocks (fixed order;
 * loss = sum(partials) * inv_denom with inv_denom = 1 / (sum(mask) F)); grad_eps (nullable) = d loss / d eps. */
size_t gtts_score_loss_partials(int B, int F, int T);
int gtts_score_loss(const float *eps, const float *z_masked, const float *t, float beta_min, float beta_max, float inv_denom,
                    float *partials, float *grad_eps, int B, int F, int T, gtts_stream_t stream);
/* Block's convolution for training: y = Conv2d_3x3(x * mask) + bias with weights packed by gtts_conv3x3_pack (transposed = 0).
 * x [B,cin,H,W], mask [B,W] (columns), y [B,cout,H,W]; cout 64 or a multiple of 128.
 * x1 (nullable) / c0: the input is the channel concatenation of x [B,c0,H,W] and x1 [B,cin-c0,H,W], read in place (torch.cat of the
 * up path, diffusion.py:166); c0 a multiple of 16 here, of 64 in the weight gradient.  Without x1, c0 is ignored.
 * omask (nullable): [B,W] column mask multiplied into the output.  The data gradient is this call on dy with weights packed
 * transposed = 1 (cin / cout swapped), an all-ones mask, a zero bias and the forward mask as omask. */
size_t gtts_conv3x3_packed_bytes(int cin, int cout);
int gtts_conv3x3_pack(const float *w, void *packed, int cin, int cout, int transposed, gtts_stream_t stream);
int gtts_conv3x3_masked(const float *x, const float *x1, int c0, const float *mask, const float *omask, const void *packed,
                        const float *bias, float *y, int B, int cin, int cout, int H, int W, gtts_stream_t stream);
/* Its weight / bias gradient dw [cout][cin][3][3], db [cout] (nullable), both overwritten: an LDS-tiled reduction in a fixed order
 * (no atomics); cin and cout multiples of 64.  workspace: gtts_conv3x3_wgrad_workspace_bytes(...) bytes of device memory (per-slice
 * partial tiles).  The kernel addresses a call's tensors with 32-bit byte offsets: B * max(cin, cout) * H * W < 2^29 (GTTS_E_SHAPE),
 * as for gtts_conv1x1_wgrad. */
size_t gtts_conv3x3_wgrad_workspace_bytes(int B, int cin, int cout, int H, int W);
int gtts_conv3x3_wgrad(const float *x, const float *x1, int c0, const float *mask, const float *dy, float *dw, float *db,
                       void *workspace, size_t workspace_bytes, int B, int cin, int cout, int H, int W, gtts_stream_t stream);

/* Block's GroupNorm + Mish + mask for training (Grad-TTS/model/diffusion.py:53-58,13-15), with ResnetBlock's time term (:75-76):
 * out = Mish(GroupNorm(y)) * mask + tb[b,c].  y, out [B,C,H,W]; gamma, beta [C]; mask [B,W] (columns); tb [B][C] (nullable: no term).
 * stats: gtts_gn_mish_stats_floats(B, groups) floats, 8-byte aligned; its first [B][groups][2] = (mean, 1/sqrt(var + eps)) are
 * written by the forward call (the rest is its reduction scratch) and read by the backward call, which overwrites dy [B,C,H,W],
 * dgamma [C], dbeta [C] and dtb [B][C] (nullable); scratch: gtts_gn_mish_scratch_bytes(B, C) bytes of device memory. */
size_t gtts_gn_mish_stats_floats(int B, int groups);
int gtts_gn_mish_forward(const float *y, const float *gamma, const float *beta, const float *mask, const float *tb, float *out,
                         float *stats, int B, int C, int H, int W, int groups, float eps, gtts_stream_t stream);
size_t gtts_gn_mish_scratch_bytes(int B, int C);
int gtts_gn_mish_backward(const float *dout, const float *y, const float *gamma, const float *beta, const float *mask,
                          const float *stats, float *dy, float *dgamma, float *dbeta, float *dtb, void *scratch, int B, int C, int H,
                          int W, int groups, gtts_stream_t stream);

/* ---- training hot path, the rest of the score network (Grad-TTS/model/diffusion.py:19-108,140-176) -----------------------
 * Every tensor-sized op of Diffusion.compute_loss's forward and backward (Upsample's gradients run as stride-1 3x3 operations
 * over gtts_space_to_depth2 planes: no MIOpen / rocBLAS kernel is left in the step). */
/* 1x1 convolutions (res_conv, to_qkv, to_out: diffusion.py:70,87-88): y = Conv2d_1x1(x * mask) + bias; the data gradient is the
 * same call on dy with weights packed transposed = 1 (the mask then applies to dy: columns do not mix); weight gradient
 * dw [cout][cin], db [cout] (nullable); mask [B,W] (nullable in the weight gradient).  cin, cout multiples of 64. */
size_t gtts_conv1x1_packed_bytes(int cin, int cout);
int gtts_conv1x1_pack(const float *w, void *packed, int cin, int cout, int transposed, gtts_stream_t stream);
int gtts_conv1x1_masked(const float *x, const float *mask, const void *packed, const float *bias, float *y, int B, int cin,
                        int cout, int H, int W, gtts_stream_t stream);
size_t gtts_conv1x1_wgrad_workspace_bytes(int B, int cin, int cout, int H, int W);
int gtts_conv1x1_wgrad(const float *x, const float *mask, const float *dy, float *dw, float *db, void *workspace,
                       size_t workspace_bytes, int B, int cin, int cout, int H, int W, gtts_stream_t stream);
/* First-layer weight gradient (stacked (mu, x[, spk]) input: cin 2 or 3; ksize 3 or 1): dw [cout][cin][k][k], db [cout]. */
size_t gtts_conv_wgrad_small_scratch_floats(int B, int cin, int cout, int ksize);
int gtts_conv_wgrad_small(const float *x, const float *mask, const float *dy, float *dw, float *db, float *scratch, int B, int cin,
                          int cout, int H, int W, int ksize, gtts_stream_t stream);
/* Downsample (up = 0: Conv2d 3x3 stride 2 pad 1, w [cout][cin][3][3]) / Upsample (up = 1: ConvTranspose2d 4x4 stride 2 pad 1,
 * w [cin][cout][4][4]) of x * mask (diffusion.py:19-34); x [B,cin,H,W], mask [B,W], y [B,cout,H/2,W/2] or [B,cout,2H,2W].
 * Downsample's data gradient is the up = 1 call on dy with its forward weight zero-padded to 4x4. */
size_t gtts_conv_resample_packed_bytes(int cin, int cout, int up);
int gtts_conv_resample_pack(const float *w, void *packed, int cin, int cout, int up, gtts_stream_t stream);
int gtts_conv_resample(const float *x, const float *mask, const void *packed, const float *bias, float *y, int B, int cin, int cout,
                       int H, int W, int up, gtts_stream_t stream);
/* Which kernel instance a forward / data-gradient convolution of the training path runs (additive): the name a demangler prints
 * ("gtts::conv_mfma_kernel<0, 1, 4, 2, 1, 1, 0, 2, 1, float, 2, 0>"), taken from the dispatch that launches it -- the entry point's
 * shape checks, its launch arguments without pointers, and the launcher describing instead of launching.  Host only: no device call.
 * kind 0: gtts_conv3x3_masked, 1: gtts_conv1x1_masked, 2: gtts_conv7x7_masked, 3: gtts_conv_resample (`up` is read for kind 3 only).
 * B, cin, cout, H, W: those of the call asked about (a data gradient is the call with the forward's cin and cout swapped; Downsample's
 * is an up = 1 call on the halved plane).  c0 in (0, cin): two sources (kind 0 only); 0 or cin: one.  buf [n] receives the name.
 *   GTTS_E_NULL: buf NULL or n = 0; GTTS_E_CONFIG: unknown kind, two sources for a kind other than 0, no instance takes the call;
 *   GTTS_E_SHAPE: what the entry point refuses; GTTS_E_WORKSPACE: n too small. */
int gtts_conv_train_kernel_name(int kind, int B, int cin, int c0, int cout, int H, int W, int up, char *buf, size_t n);
/* ABI 4: every weight pack of a training step in ONE launch.  item.kind: 0 Block 3x3 (gtts_conv3x3_pack), 1 1x1 (gtts_conv1x1_pack),
 * 2 Downsample, 3 Upsample (gtts_conv_resample_pack), 4 Downsample's data gradient (its forward weight [cout][cin][3][3] packed as the
 * zero-padded 4x4 transposed convolution; cin / cout those of the GRADIENT convolution); transposed as in the single-pack calls
 * (kinds 0 / 1).  gtts_pack_batch_describe turns n items into a descriptor table in HOST memory (gtts_pack_batch_desc_bytes(n)
 * bytes) and returns the launch width; the caller keeps a device copy of the table (addresses are stable across steps) and calls
 * gtts_pack_batch at the top of every step. */
typedef struct gtts_pack_item { const float *w; void *packed; int kind, cin, cout, transposed; } gtts_pack_item;
size_t gtts_pack_batch_desc_bytes(int n);
int gtts_pack_batch_describe(const gtts_pack_item *items, int n, void *desc_host, int *grid_x);
int gtts_pack_batch(const void *desc_dev, int n, int grid_x, gtts_stream_t stream);
int gtts_zero_insert2(const float *in, float *out, int B, int C, int h, int w, gtts_stream_t stream);
/* out [B,4C,h,w] = the four stride-2 phases of in [B,C,2h,2w], channel block (pr * 2 + pc) = rows 2y + 1 - pr, columns 2x + 1 - pc:
 * Upsample's data / weight gradient are the 3x3 stride-1 convolution / weight gradient over these planes. */
int gtts_space_to_depth2(const float *in, float *out, int B, int C, int h, int w, gtts_stream_t stream);
/* LinearAttention between its two 1x1 convolutions (diffusion.py:90-100): qkv [B][384][N] -> out [B][128][N]; ctx [B][4][32][32]
 * and stat [B][4][32][2] (softmax row maximum, reciprocal sum) are kept for the backward call, which writes dqkv [B][384][N];
 * dctx [B][4][32][32], rdot [B][4][32]: outputs used as scratch; scratch: gtts_attn_train_scratch_floats(B, N) floats. */
size_t gtts_attn_train_scratch_floats(int B, int N);
int gtts_attn_train_forward(const float *qkv, float *out, float *ctx, float *stat, float *scratch, int B, int N, gtts_stream_t stream);
int gtts_attn_train_backward(const float *qkv, const float *dout, const float *ctx, const float *stat, float *dqkv, float *dctx,
                             float *rdot, float *scratch, int B, int N, gtts_stream_t stream);
/* Residual(Rezero(f)): y = f * g + x, g one device scalar (diffusion.py:40-46,103-108); backward df = dy * g, dg = sum(dy * f);
 * n floats, a multiple of 4; scratch: gtts_rezero_scratch_bytes(n) bytes. */
int gtts_rezero_forward(const float *f, const float *x, const float *g, float *y, size_t n, gtts_stream_t stream);
size_t gtts_rezero_scratch_bytes(size_t n);
int gtts_rezero_backward(const float *dy, const float *f, const float *g, float *df, float *dg, void *scratch, size_t n,
                         gtts_stream_t stream);
/* out = a + b * mask over [B,C,H,W], mask [B,W] (a nullable: b * mask; mask nullable: a + b); b_cstride > 0: b is a C-channel
 * slice of a contiguous tensor with b_cstride channels (the split of a concatenation's gradient). */
int gtts_add_masked(const float *a, const float *b, const float *mask, float *out, int B, int C, int H, int W, int b_cstride,
                    gtts_stream_t stream);
/* final_conv (C -> 1) with both masks (diffusion.py:175-176): out [B,1,H,W] = (sum_c w[c] x[b,c] m + bias) m and its gradients
 * dx [B,C,H,W], dw [C], db [1]; scratch: gtts_final_conv_scratch_floats(B, C, H, W) floats. */
int gtts_final_conv_forward(const float *x, const float *w, const float *bias, const float *mask, float *out, int B, int C, int H,
                            int W, gtts_stream_t stream);
size_t gtts_final_conv_scratch_floats(int B, int C, int H, int W);
int gtts_final_conv_backward(const float *x, const float *w, const float *mask, const float *dout, float *dx, float *dw, float *db,
                             float *scratch, int B, int C, int H, int W, gtts_stream_t stream);

/* ---- ABI 6: DiffVC decoder training, RefBlock's InstanceNorm2d(affine) + GLU(dim=1) pair (DiffVC/model/modules.py:128-157) ----------
 * y [B,2C,H,W] (the block's convolution output), gamma / beta [2C]; out [B,C,H,W] = IN(y[:, :C]) * sigmoid(IN(y[:, C:])), statistics
 * per (sample, channel) plane over H x W (biased variance, eps).  stats: gtts_in_glu_stats_floats(B, C) floats written by the forward
 * call ((mean, rstd) of both halves) and read by the backward call, which writes dy [B,2C,H,W], dgamma [2C], dbeta [2C];
 * scratch: gtts_in_glu_scratch_floats(B, C) floats. */
size_t gtts_in_glu_stats_floats(int B, int C);
size_t gtts_in_glu_scratch_floats(int B, int C);
int gtts_in_glu_forward(const float *y, const float *gamma, const float *beta, float *out, float *stats, int B, int C, int H, int W,
                        float eps, gtts_stream_t stream);
int gtts_in_glu_backward(const float *dout, const float *y, const float *gamma, const float *beta, const float *stats, float *dy,
                         float *dgamma, float *dbeta, float *scratch, int B, int C, int H, int W, gtts_stream_t stream);

/* ---- ABI 6 (additive): DiffVC "average voice" encoder training, the PostNet (DiffVC/model/postnet.py:15-53, FwdDiffusion.compute_loss
 * of DiffVC/train_enc.py) --------------------------------------------------------------------------------------------------------
 * Block's 7x7 convolution: y = Conv2d_7x7(x * mask, padding 3) + bias with weights packed by gtts_conv7x7_pack (transposed = 0);
 * the data gradient is the same call on dy with weights packed transposed = 1 (cin / cout swapped), an all-ones mask, a zero bias
 * and omask = the column mask (d loss / d x of the masked convolution in one pass; omask nullable).  x [B,cin,H,W], mask / omask
 * [B,W].  The weight / bias gradient gtts_conv7x7_wgrad overwrites dw [cout][cin][7][7] and db [cout] (nullable): split-bf16 MFMA,
 * deterministic; workspace: gtts_conv7x7_wgrad_workspace_bytes(...) bytes of device memory.  cin and cout multiples of 64
 * (GTTS_E_CONFIG), B * max(cin, cout) * H * W < 2^29 (GTTS_E_SHAPE); arguments are checked before the device is touched. */
size_t gtts_conv7x7_packed_bytes(int cin, int cout);
int gtts_conv7x7_pack(const float *w, void *packed, int cin, int cout, int transposed, gtts_stream_t stream);
int gtts_conv7x7_masked(const float *x, const float *mask, const float *omask, const void *packed, const float *bias, float *y, int B,
                        int cin, int cout, int H, int W, gtts_stream_t stream);
size_t gtts_conv7x7_wgrad_workspace_bytes(int B, int cin, int cout, int H, int W);
int gtts_conv7x7_wgrad(const float *x, const float *mask, const float *dy, float *dw, float *db, void *workspace, size_t workspace_bytes,
                       int B, int cin, int cout, int H, int W, gtts_stream_t stream);
/* PostNet's single-channel 1x1 convolutions (init_conv 1 -> C, final_conv C -> 1) and their gradients:
 *   expand    out [B,C,F,T] = w[c] * x[b,f,t] * mask[b,t] + bias[c]           (init_conv forward; final_conv's data gradient, zero bias)
 *   collapse  out [B,F,T]   = sum_c w[c] * x[b,c,f,t] * mask[b,t] + bias[0]    (final_conv forward; init_conv's data gradient, zero bias)
 *   chan_dot  dot[c] = sum_{b,f,t} a[b,c,f,t] * v[b,f,t] * mask[b,t],  sum[c] = sum_{b,f,t} a[b,c,f,t]   (v, mask, one of dot / sum
 *             nullable; fixed-order two-pass reduction; scratch: gtts_postnet_chan_dot_scratch_floats(B, C, F, T) floats) */
int gtts_postnet_expand(const float *x, const float *mask, const float *w, const float *bias, float *out, int B, int C, int F, int T,
                        gtts_stream_t stream);
int gtts_postnet_collapse(const float *x, const float *mask, const float *w, const float *bias, float *out, int B, int C, int F, int T,
                          gtts_stream_t stream);
size_t gtts_postnet_chan_dot_scratch_floats(int B, int C, int F, int T);
int gtts_postnet_chan_dot(const float *a, const float *v, const float *mask, float *dot, float *sum, float *scratch, int B, int C, int F,
                          int T, gtts_stream_t stream);

/* ---- ABI 6 (additive): log-mel front end, waveform -> the mel every other entry point takes in: mel_spectrogram(..., center=False) of
 * Grad-TTS/hifi-gan/meldataset.py:51-74 (DiffVC's get_mel uses an identical copy) in one launch (csrc/mel.hip) ----------------------
 * Each row of wav [B,L] is reflect-padded by p = (n_fft - hop_size) / 2 on both sides (needs L > p), cut into frames of n_fft samples at
 * stride hop_size (T = (L + 2p - n_fft) / hop_size + 1; a tail shorter than a frame is dropped), windowed with the periodic Hann window
 * of win_size samples (centred in the frame when win_size < n_fft, as torch.stft does), transformed (one-sided DFT, unnormalised),
 * mag = sqrt(re^2 + im^2 + 1e-9), projected on librosa's default mel filterbank (slaney scale and normalisation, computed here in
 * float64 and rounded to fp32) and compressed: out [B,num_mels,T] = log(max(W mag, 1e-5)).
 * Supported (else GTTS_E_CONFIG): n_fft a power of two in [256, 2048], 1 <= win_size <= n_fft, 1 <= hop_size <= n_fft with
 * n_fft - hop_size even, 1 <= num_mels <= 128, 0 <= fmin < fmax <= sampling_rate / 2.
 * The handle is host metadata; gtts_mel_pack copies its tables (window, twiddles, filterbank: host float64 -> fp32) into the caller's
 * blob of gtts_mel_packed_bytes bytes.  gtts_mel_forward takes no workspace and is a single kernel launch on `stream`.
 * lengths (nullable, device int32 [B]): row b is the utterance wav[b, :lengths[b]] -- reflected about ITS ends -- and frames at or
 * beyond gtts_mel_frames(lengths[b]) are written as 0 (the mel padding of the reference collate functions); a length outside (p, L] is
 * clamped to L from above and yields an all-zero row from below.  A frame's value depends on its own n_fft samples alone, never on B
 * or on its position in the batch. */
typedef struct gtts_mel_cfg {
    int n_fft;           /* 1024                                             */
    int num_mels;        /* 80                                               */
    int sampling_rate;   /* 22050                                            */
    int hop_size;        /* 256                                              */
    int win_size;        /* 1024                                             */
    double fmin;         /* 0                                                */
    double fmax;         /* 8000                                             */
} gtts_mel_cfg;
typedef struct gtts_mel gtts_mel;     /* host-side metadata only */
int gtts_mel_create(const gtts_mel_cfg *cfg, gtts_mel **out);
void gtts_mel_destroy(gtts_mel *mel);
/* T for rows of L samples, or GTTS_E_SHAPE when L <= p or the padded row holds no whole frame */
int gtts_mel_frames(const gtts_mel *mel, int L);
size_t gtts_mel_packed_bytes(const gtts_mel *mel);
int gtts_mel_pack(const gtts_mel *mel, void *packed, gtts_stream_t stream);
/* the filterbank W [num_mels][n_fft / 2 + 1] as fp32 into HOST memory; touches no device */
int gtts_mel_filterbank(const gtts_mel *mel, float *host_out);
int gtts_mel_forward(const gtts_mel *mel, const void *packed, const float *wav, const int *lengths, float *out, int B, int L,
                     gtts_stream_t stream);
/* ---- ABI 7 (additive): the input gradient of gtts_mel_forward (csrc/mel_train.hip) -- what the HiFi-GAN mel loss sends to the generator.
 * dmel [B,num_mels,T] -> dwav [B,L] for the same wav, lengths and blob as the forward; nothing else is kept from the forward, the frame
 * spectra are formed again.  The clip passes the gradient where W mag >= 1e-5 (torch's clamp), frames at or beyond a row's own count and
 * samples at or beyond lengths[b] get 0.  Two launches (windowed frame gradients [B][T][n_fft] into the workspace of
 * gtts_mel_backward_workspace_bytes(B, L) bytes, then a gather per sample in a fixed order), no floating-point atomics: two calls
 * return the same bits, and a row's gradient depends on that row alone.  Refused before any launch: null pointers (GTTS_E_NULL), B
 * outside [1, 65535] and every L gtts_mel_frames refuses (GTTS_E_SHAPE), a short workspace (GTTS_E_WORKSPACE). */
size_t gtts_mel_backward_workspace_bytes(const gtts_mel *mel, int B, int L);      /* 0 for a null handle, B <= 0 or a refused L */
int gtts_mel_backward(const gtts_mel *mel, const void *packed, const float *wav, const int *lengths, const float *dmel, float *dwav,
                      void *workspace, size_t workspace_bytes, int B, int L, gtts_stream_t stream);

/* ---- ABI 6 (additive): DiffVC speaker encoder, the 256-d embedding `c` of DiffVC.forward (DiffVC/speaker_encoder/encoder/model.py:43-63,
 * inference.py:150-151) on csrc/spk.hip ---------------------------------------------------------------------------------------------
 * torch.nn.LSTM(n_mels -> hidden, layers, batch_first=True) with zero initial state (gate order i, f, g, o; c_t = s(f) c_{t-1} + s(i) tanh(g),
 * h_t = s(o) tanh(c_t); both biases), then embeds = r / ||r||_2 with r = relu(W h_T + b) of the last layer -- no epsilon: an all-zero r
 * gives a NaN row, as in the reference.  fp32 arithmetic throughout (v_mfma_f32_16x16x4_f32 = an fmaf chain, expf / tanhf).
 * Sequences are addressed inside frames [U][T_total][n_mels] (fp32, contiguous) so that partial utterances are never stacked: sequence
 * n in [0, U P) is rows (n % P) S ... (n % P) S + T - 1 of utterance n / P; P = 1, S = 0, T = T_total is the plain batched call.
 * (P - 1) S + T > T_total is refused with GTTS_E_SHAPE before the device is touched, as is U P T * 4 hidden >= 2^31.
 * Outputs: embeds [U P][embed]; hidden_out (nullable) [U P][hidden] = h_T of the last layer; utt_embeds (nullable) [U][embed] =
 * m / ||m||_2 with m the mean of the utterance's P embeddings.  A sequence's result does not depend on U, P or its position.
 * Supported (else GTTS_E_CONFIG): hidden = 256, n_mels a multiple of 4 in [4, 1024], 1 <= layers <= 8, 1 <= embed <= 4096.
 * Parameters in the module's state_dict order: lstm.weight_ih_l{k}, lstm.weight_hh_l{k}, lstm.bias_ih_l{k}, lstm.bias_hh_l{k} per layer,
 * then linear.weight, linear.bias (GTTS_E_PARAMS on a count mismatch).  Per layer one input-projection launch over all U P T rows and one
 * persistent recurrence launch (a workgroup per 16 sequences, no workgroup waits on another), then the head: 2 layers + 1 (+ 1) launches. */
typedef struct gtts_spk_cfg {
    int n_mels;          /* 40  */
    int hidden;          /* 256 */
    int layers;          /* 3   */
    int embed;           /* 256 */
} gtts_spk_cfg;
typedef struct gtts_spk gtts_spk;     /* host-side metadata only */
int gtts_spk_create(const gtts_spk_cfg *cfg, gtts_spk **out);
void gtts_spk_destroy(gtts_spk *spk);
int gtts_spk_num_params(const gtts_spk *spk);
int gtts_spk_param_info(const gtts_spk *spk, int i, const char **name, int *rank, int dims[4]);
size_t gtts_spk_packed_bytes(const gtts_spk *spk);
int gtts_spk_pack(const gtts_spk *spk, const void *const *param_ptrs, int n_params, void *packed, gtts_stream_t stream);
/* bytes for N = U P sequences of T frames (0 for a shape gtts_spk_forward refuses) */
size_t gtts_spk_workspace_bytes(const gtts_spk *spk, int N, int T);
int gtts_spk_forward(const gtts_spk *spk, const void *packed, const float *frames, int U, int T_total, int P, int S, int T, float *embeds,
                     float *hidden_out, float *utt_embeds, void *workspace, size_t workspace_bytes, gtts_stream_t stream);

/* ---- ABI 6 (additive): training of the speaker encoder (DiffVC/speaker_encoder/encoder/train.py, model.py:35-137) on csrc/spk_train.hip --
 * fp32 on the same MFMA; every reduction runs in a fixed order and nothing is accumulated with atomics: a call repeated gives the same bits.
 * gtts_spktrain_forward is gtts_spk_forward (P = 1, S = 0, T = T_total; the blob of gtts_spk_pack) keeping what the backward needs in the
 * caller's `saved` buffer of gtts_spktrain_saved_bytes(N, T) bytes: per layer the activated gates [N T][4 hidden], the cell states and the
 * hidden sequence [N T][hidden] each, then h_T [N][hidden] and the head before its L2 norm [N][embed], every part rounded up to 256 bytes
 * (layers 6 N T hidden 4 bytes and a little: 1 888 747 520 bytes at N = 640, T = 160).  Its embeds equal gtts_spk_forward's bit for bit.
 * gtts_spktrain_backward takes d_embeds [N][embed], the same frames, the saved buffer (which it CONSUMES: the gate gradients are written over
 * the gates, so one backward per forward), the blob of gtts_spktrain_pack (gtts_spktrain_packed_bytes bytes: W_hh^T and W_ih^T in MFMA
 * fragment order, linear.weight; the same parameter pointers as gtts_spk_pack) and a workspace of gtts_spktrain_workspace_bytes(N, T)
 * bytes, and writes one gradient per parameter through grads[i], i in gtts_spk_param_info order, each of the parameter's shape
 * (bias_ih and bias_hh receive the same values).  There is no gradient for the frames.  Per layer, top down: one persistent recurrence
 * launch (a workgroup per 16 sequences walking t = T - 1 ... 0; no workgroup waits on another), the data gradient dZ W_ih for the layer
 * below, and the weight gradients dZ^T [X | H_prev] over slices of the N T rows (at least 256 rows a slice, at most 16 slices) added in
 * ascending order.  Refused on the host before any launch: null arguments GTTS_E_NULL, a gradient count other than the parameter count
 * GTTS_E_PARAMS, N or T < 1 or N T 4 hidden >= 2^31 GTTS_E_SHAPE, a short saved buffer or workspace GTTS_E_WORKSPACE; the three size
 * functions return 0 for a null handle or a refused shape. */
size_t gtts_spktrain_packed_bytes(const gtts_spk *spk);
size_t gtts_spktrain_saved_bytes(const gtts_spk *spk, int N, int T);
size_t gtts_spktrain_workspace_bytes(const gtts_spk *spk, int N, int T);
int gtts_spktrain_pack(const gtts_spk *spk, const void *const *param_ptrs, int n_params, void *packed_train, gtts_stream_t stream);
int gtts_spktrain_forward(const gtts_spk *spk, const void *packed, const float *frames, int N, int T, float *embeds, void *saved,
                           size_t saved_bytes, gtts_stream_t stream);
int gtts_spktrain_backward(const gtts_spk *spk, const void *packed_train, const float *frames, const float *d_embeds, void *saved,
                      size_t saved_bytes, float *const *grads, int n_grads, void *workspace, size_t workspace_bytes, int N, int T,
                      gtts_stream_t stream);
/* GE2E loss of embeds [S][U][E] (model.py:65-126): inclusive centroids (mean over U, normalised), exclusive centroids ((sum - e) / (U - 1),
 * normalised), sim[s u][j] = w <e_su, centroid_j> + b with the exclusive centroid of (s, u) where j = s, loss = the mean cross-entropy of
 * the S U rows against their speaker.  w, b: device scalars.  Outputs: sim [S U][S], loss [1], and -- each nullable -- d_embeds [S][U][E],
 * dw [1], db [1] for a loss gradient of 1.  No epsilon; U = 1 is not special-cased (0 / 0 = NaN, as in the reference).  One launch of one
 * workgroup; workspace of gtts_ge2e_workspace_bytes(S, U, E) bytes (0 for a refused shape).  GTTS_E_SHAPE: S, U or E < 1, S > 1024, or
 * S U max(S, E) >= 2^31. */
size_t gtts_ge2e_workspace_bytes(int S, int U, int E);
int gtts_ge2e_loss(const float *embeds, const float *w, const float *b, int S, int U, int E, float *sim, float *loss, float *d_embeds,
                   float *dw, float *db, void *workspace, size_t workspace_bytes, gtts_stream_t stream);

/* ---- ABI 6 (additive): Fast Griffin-Lim, log-mel -> waveform without a vocoder checkpoint: FastGL / PseudoInversion /
 * InitialReconstruction of DiffVC/model/utils.py:42-110 on csrc/fgl.hip -------------------------------------------------------------
 * K = n_fft / 2 + 1, w = the periodic Hann window of n_fft samples (win_length = n_fft), m = momentum, L = hop_size (T - 1).
 *   c [B,K,T] = P exp(logmel), P [K][n_mels] the caller's pseudo-inverse of the mel filterbank (the library does no SVD); c may be
 *   negative and is used as it is;  x0 = istft(c + 0i);  then n_iters times
 *   s = stft(x),  a = s / sqrt(max(re^2 + im^2, 1e-8)),  x = istft(c (a + m (a - a_prev))),  a_prev = a   (a_prev = 0 at first).
 * stft: center = True, reflect pad n_fft / 2 (needs L > n_fft / 2), one-sided, unnormalised.  istft: per-frame c2r transform scaled
 * 1 / n_fft (imaginary parts of DC and Nyquist ignored), times w, overlap-added at stride hop_size, divided by the envelope
 * sum_t w^2[j - t hop_size], n_fft / 2 trimmed from both ends.  fp32 throughout; tables host float64 -> fp32; no device sin / cos.
 * Supported (else GTTS_E_CONFIG): n_fft a power of two in [256, 2048], 1 <= hop_size <= n_fft / 2 (the envelope is then positive
 * everywhere after the trim), 1 <= n_mels <= 128, 0 <= momentum < 1.
 * The handle is host metadata; gtts_fgl_pack copies its tables and the caller's HOST matrix into the caller's blob of
 * gtts_fgl_packed_bytes bytes (it waits for the copy).  Every call takes a workspace of gtts_fgl_workspace_bytes(B, T) bytes.
 * [B,K,T,2] is the memory of a torch complex64 [B,K,T].  Launches on `stream`: init = projection, first inverse transform, one that
 * materialises x0; step = one transform launch + one that materialises x_out; forward = projection, first inverse transform, ONE
 * launch per iteration, one that materialises wav -- between iterations x exists only as windowed inverse frames in the workspace,
 * and launches are ordered by stream order alone (no workgroup waits for another, no cooperative launch).  No floating-point atomics:
 * the at most ceil(n_fft / hop_size) overlapping frames of a sample are summed in ascending frame order, the mel projection in a
 * fixed order.  gtts_fgl_forward(n_iters = n) equals gtts_fgl_init followed by n gtts_fgl_step bit for bit; n_iters = 0 returns x0.
 * A row's result depends on that row's mel alone, never on B or on its position in the batch. */
typedef struct gtts_fgl_cfg {
    int n_fft;           /* 1024  */
    int n_mels;          /* 80    */
    int hop_size;        /* 256   */
    double momentum;     /* 0.99  */
} gtts_fgl_cfg;
typedef struct gtts_fgl gtts_fgl;     /* host-side metadata only */
int gtts_fgl_create(const gtts_fgl_cfg *cfg, gtts_fgl **out);
void gtts_fgl_destroy(gtts_fgl *fgl);
/* L = hop_size (T - 1) for mels of T frames, or GTTS_E_SHAPE when that is <= n_fft / 2 (the message names the smallest T) */
int gtts_fgl_samples(const gtts_fgl *fgl, int T);
size_t gtts_fgl_packed_bytes(const gtts_fgl *fgl);
/* inv_basis_host: P [K][n_mels] fp32 in HOST memory */
int gtts_fgl_pack(const gtts_fgl *fgl, const float *inv_basis_host, void *packed, gtts_stream_t stream);
size_t gtts_fgl_workspace_bytes(const gtts_fgl *fgl, int B, int T);
/* logmel [B,n_mels,T] -> c [B,K,T], x0 [B,L] */
int gtts_fgl_init(const gtts_fgl *fgl, const void *packed, const float *logmel, float *c, float *x0, void *workspace,
                  size_t workspace_bytes, int B, int T, gtts_stream_t stream);
/* one iteration: c [B,K,T], x_in [B,L], a_prev [B,K,T,2] -> x_out [B,L], a [B,K,T,2] (x_out / a must not alias x_in / a_prev) */
int gtts_fgl_step(const gtts_fgl *fgl, const void *packed, const float *c, const float *x_in, const float *a_prev, float *x_out, float *a,
                  void *workspace, size_t workspace_bytes, int B, int T, gtts_stream_t stream);
/* logmel [B,n_mels,T] -> wav [B,L] after n_iters >= 0 iterations */
int gtts_fgl_forward(const gtts_fgl *fgl, const void *packed, const float *logmel, float *wav, void *workspace, size_t workspace_bytes,
                     int B, int T, int n_iters, gtts_stream_t stream);

/* ---- ABI 6 (additive): waveform front end of the DiffVC speaker encoder, waveform -> what gtts_spk_forward takes in: the batch functions of
 * DiffVC/speaker_encoder/encoder/audio.py (preprocess_wav_batch :50-58, wav_to_mel_spectrogram_batch :76-89, normalize_volume_batch
 * :101-114) on csrc/wav.hip -----------------------------------------------------------------------------------------------------------
 * Resample = torchaudio.transforms.Resample(source_sr, sampling_rate) with its defaults (sinc_interp_hann): with g = gcd of the rates,
 *   o = source_sr / g, n = sampling_rate / g, base = min(o, n) rolloff, w = ceil(lowpass_filter_width o / base), phase p in [0, n) and
 *   tap j in [0, 2 w + o):  t = clamp((-p / n + (j - w) / o) base, -lpw, lpw),
 *   k[p][j] = (base / o) cos^2(t pi / (2 lpw)) sinc(t)  (float64, rounded to fp32);  each row is zero-padded by w on the left and w + o
 *   on the right;  out[q n + p] = sum_j k[p][j] xpad[q o + j], cut to gtts_wav_resampled_length(L) = ceil(n L / o) samples.  Taps on
 *   the clamp (1e-49 in float64, 0 in fp32) are left out: gtts_wav_span taps per phase remain, summed in ascending j.
 *   partials [B][gtts_wav_tiles(L')] receives the sum of out^2 over every tile of 1024 output samples.
 * Normalise: change = target_dBFS - 10 log10(mean(x^2)); gain = 10^(change / 20) where change > 0 (mode 1, increase only) or change < 0
 *   (mode 2, decrease only), else exactly 1 (mode 0: always); out = wav * gain (out may be wav).  An all-zero row gives 0 * inf = NaN
 *   under mode 1 and stays 0 under modes 0 and 2 (the reference's 1 + mask (gain - 1) makes it NaN in every mode).  partials: the
 *   resampler's tile sums of THIS wav, or NULL -- the same sums are then formed in workspace (gtts_wav_workspace_bytes(B, L) bytes) by
 *   one more launch, and the result is the same bit for bit.
 * Power mel: reflect pad n_fft / 2 (needs L > n_fft / 2), frames of n_fft samples at stride hop_size (T = gtts_wav_frames(L) = 1 + L /
 *   hop_size), periodic Hann window of n_fft samples, one-sided DFT (unnormalised), re^2 + im^2, librosa's default mel filterbank
 *   (slaney; float64 -> fp32): out [B,T,n_mels], frame-major.  No sqrt, no epsilon, no log.  One launch, no workspace.
 * fp32 throughout, tables host float64 -> fp32 (gtts_wav_pack copies them into the caller's blob of gtts_wav_packed_bytes bytes), no
 * floating-point atomics, every sum in a fixed order: a value depends on its own row alone, never on B or its position in the batch.
 * Supported (else GTTS_E_CONFIG): o, n <= 1024; 1 <= lowpass_filter_width <= 64; 0 < rolloff <= 1; n_fft even in [64, 1024];
 * 1 <= hop_size <= n_fft; 1 <= n_mels <= 128; 0 <= fmin < fmax <= sampling_rate / 2.  gtts_wav_resample on a handle with source_sr ==
 * sampling_rate is GTTS_E_CONFIG.  Refused with GTTS_E_SHAPE before the device is touched: L < 1, L <= n_fft / 2 for the mel, B outside
 * [1, 65535], B L, B L' or B T n_mels >= 2^31. */
typedef struct gtts_wav_cfg {
    int source_sr;              /* 22050 */
    int sampling_rate;          /* 16000 */
    int n_fft;                  /* 400   */
    int hop_size;               /* 160   */
    int n_mels;                 /* 40    */
    int lowpass_filter_width;   /* 6     */
    double rolloff;             /* 0.99  */
    double fmin;                /* 0     */
    double fmax;                /* 8000  */
} gtts_wav_cfg;
typedef struct gtts_wav gtts_wav;     /* host-side metadata only */
int gtts_wav_create(const gtts_wav_cfg *cfg, gtts_wav **out);
void gtts_wav_destroy(gtts_wav *wav);
/* L' = ceil(n L / o), T = 1 + L / hop_size, tiles of 1024 samples in a row of L -- or GTTS_E_SHAPE */
int gtts_wav_resampled_length(const gtts_wav *wav, int L);
int gtts_wav_frames(const gtts_wav *wav, int L);
int gtts_wav_tiles(const gtts_wav *wav, int L);
/* host calls, no device is touched: taps kept per phase; first_host [n] = j of every phase's first kept tap, taps_host [n][span] (zeros
 * behind a phase's last kept tap); the filterbank W [n_mels][n_fft / 2 + 1] */
int gtts_wav_span(const gtts_wav *wav);
int gtts_wav_taps(const gtts_wav *wav, int *first_host, float *taps_host);
int gtts_wav_filterbank(const gtts_wav *wav, float *host_out);
size_t gtts_wav_packed_bytes(const gtts_wav *wav);
int gtts_wav_pack(const gtts_wav *wav, void *packed, gtts_stream_t stream);
/* bytes gtts_wav_normalize needs without partials (0 for a shape it refuses) */
size_t gtts_wav_workspace_bytes(const gtts_wav *wav, int B, int L);
/* wav [B,L] -> out [B,L'], partials [B][gtts_wav_tiles(L')] */
int gtts_wav_resample(const gtts_wav *wav, const void *packed, const float *in, float *out, float *partials, int B, int L,
                      gtts_stream_t stream);
/* in [B,L] -> out [B,L] (may alias in); partials [B][gtts_wav_tiles(L)] or NULL (then workspace) */
int gtts_wav_normalize(const gtts_wav *wav, const float *in, const float *partials, double target_dBFS, int mode, float *out,
                       void *workspace, size_t workspace_bytes, int B, int L, gtts_stream_t stream);
/* in [B,L] -> out [B,T,n_mels] */
int gtts_wav_powmel(const gtts_wav *wav, const void *packed, const float *in, float *out, int B, int L, gtts_stream_t stream);

/* ---- ABI 6 (additive): one layer of the shared 1-D convolution kernel (csrc/conv1d.h), the kernel behind every dense layer of the
 * HiFi-GAN generator and of both encoders -- the entry its per-layer tests drive; the models reach the same launcher -----------------
 *   mode 0  Conv1d(cin, cout, K, dilation, padding = (K - 1) / 2 * dilation): K odd, S = 1; weight [cout][cin][K]
 *   mode 1  ConvTranspose1d(cin, cout, K = 2 S, stride S, padding S / 2): S a power of two >= 2, dilation 1; weight [cin][cout][K]
 *   out[b][co][q] = ((sum W * (leaky_relu(x, slope) * in_mask) + bias[co]) + res), then accmode 1: accsrc + v, 2: (accsrc + v) / div,
 *   then * out_mask.  x [B][cin][Lin], out / res / accsrc [B][cout][Lin * S], in_mask [B][Lin], out_mask [B][Lin * S], bias [cout]; res,
 *   accsrc (accmode 0), in_mask and out_mask may be NULL; slope 1 = identity, 0 = ReLU.  fp32 storage, split-bf16 MFMAs, fp32 accumulate.
 * Any cin >= 1 (a last chunk of fewer than 16 channels is staged with zeros).  Refused with GTTS_E_CONFIG at create: K above 12 taps,
 * an even Conv1d kernel, K != 2 S or S not a power of two for mode 1, (K - 1) * dilation above 256 for cout * S >= 128 and above 128
 * below.  Refused with GTTS_E_SHAPE by forward / instance, on the host, before anything is launched: B or Lin < 1, a sample of
 * cout * Lin * S * 4 >= 2^31 or ceil(cin / 16) * 16 * Lin * 4 >= 2^31 bytes. */
typedef struct gtts_conv1d gtts_conv1d;     /* host-side metadata only */
int gtts_conv1d_create(int mode, int cin, int cout, int K, int dilation, int S, gtts_conv1d **out);
void gtts_conv1d_destroy(gtts_conv1d *op);
size_t gtts_conv1d_packed_bytes(const gtts_conv1d *op);
int gtts_conv1d_pack(const gtts_conv1d *op, const float *weight, void *packed, gtts_stream_t stream);
int gtts_conv1d_forward(const gtts_conv1d *op, const void *packed, const float *bias, const float *x, float *out, const float *res,
                        const float *accsrc, int accmode, float div, float slope, const float *in_mask, const float *out_mask, int B,
                        int Lin, gtts_stream_t stream);
/* host only: what forward would launch for this shape -- info = {row tile MT (128 / 64 / 32), taps per weight stage (3 / 4), staging
 * depth AITER (2 / 3), 16-channel chunks per step KCH (1 / 2), epilogue (0 buffer descriptors, 1 ConvTranspose1d 16-byte stores,
 * 2 ConvTranspose1d two 8-byte stores, 3 generic pointer path)}, from the launcher's own selection. */
int gtts_conv1d_instance(const gtts_conv1d *op, int B, int Lin, int has_res, int accmode, int has_out_mask, int info[5]);

/* ---- ABI 7 (additive): gradients of one Conv1d layer (csrc/conv1d_train.hip) -- what the encoders' Conv1d layers need under autograd.
 * Mode 0 handles only (a ConvTranspose1d handle is refused with GTTS_E_CONFIG); the handle's dilation is honoured.  For the layer
 *   y[b,co,q] = (sum_ci sum_t W[co][ci][t] x[b,ci,q+off(t)] im[b,q+off(t)] + bias[co]) om[b,q],   off(t) = (t - (K-1)/2) dilation
 * Data gradient: gtts_conv1d_forward on dy with a handle op_t created as (0, cout, cin, K, dilation, 1) -- the channels swapped --
 *   whose packed weight gtts_conv1d_pack_dgrad writes from the FORWARD module's weight [cout][cin][K]: the ordinary packed layout of
 *   op_t for W'[ci][co][t] = W[co][ci][K-1-t], in one launch; in_mask = the forward's output mask, out_mask = the forward's input mask,
 *   a zero bias.
 * Weight / bias gradient (dw [cout][cin][K], db [cout] or NULL: both overwritten, not accumulated; both masks may be NULL):
 *   dw[co][ci][t] = sum_b sum_q dy[b,co,q] om[b,q] * x[b,ci,q+off(t)] im[b,q+off(t)]      terms with q + off(t) outside [0, L) are zero
 *   db[co]        = sum_b sum_q dy[b,co,q] om[b,q]                                        (a plain fp32 sum)
 *   Split-bf16 MFMAs with fp32 accumulation, any cin, cout >= 1.  The sum over (b, q) is cut into slices of whole 64-position chunks
 *   whose partial tiles go to `workspace` (gtts_conv1d_wgrad_workspace_bytes(op, B, L) bytes; 0 for a refused call); a second launch adds
 *   the slices in ascending order.  No atomics: two calls give the same bits.
 * Refused on the host before anything is launched: null pointers GTTS_E_NULL; B or L < 1 and the sample limits of gtts_conv1d_forward
 * GTTS_E_SHAPE; a short workspace GTTS_E_WORKSPACE.  Nothing is allocated or synchronised. */
int gtts_conv1d_pack_dgrad(const gtts_conv1d *op_t, const float *weight, void *packed, gtts_stream_t stream);
size_t gtts_conv1d_wgrad_workspace_bytes(const gtts_conv1d *op, int B, int L);
int gtts_conv1d_wgrad(const gtts_conv1d *op, const float *x, const float *in_mask, const float *dy, const float *out_mask, float *dw,
                      float *db, void *workspace, size_t workspace_bytes, int B, int L, gtts_stream_t stream);
/* host only: the weight gradient's tiling at this shape, from the launcher's own arithmetic -- info = {output tile rows (co), output tile
 * columns (ci), positions per chunk, slices, chunks per slice, empty slices (slices past the last chunk: they write zeros)}; one
 * workgroup per (co tile, ci tile, tap, slice); workspace = slices * (cout * cin * K + cout) * 4 bytes. */
int gtts_conv1d_wgrad_info(const gtts_conv1d *op, int B, int L, int info[6]);

/* ---- ABI 7 (additive): the encoder-decoder gradient path of GradTTS.compute_loss (Grad-TTS/model/tts.py:101-181, train.py) -----------
 * In train.py the prior mean mu_y comes from the encoder, so the decoder's first layer needs a data gradient, the noising needs a
 * backward, and the alignment glue between MAS and the decoder runs under autograd.  All fp32 VALU kernels, no atomics, every sum in a
 * fixed order: two calls on the same inputs give the same bits.  Arguments are checked on the host before anything is launched. */
/* First-layer data gradient, the counterpart of gtts_conv_wgrad_small:
 *   dx[b,p,h,w] = mask[b,w] * sum_co sum_taps dy[b,co,h-kh+r,w-kw+r] * w[co,p,kh,kw]   (r = ksize / 2; taps outside the plane are zero)
 * dy [B,cout,H,W], w [cout][cin][k][k] (the module's layout, nothing packed), mask [B,W] -> dx [B,cin,H,W].  GTTS_E_CONFIG unless cin is
 * 2 or 3, ksize 3 or 1 and cout a multiple of 64; GTTS_E_SHAPE for B, H, W < 1 or a W too wide for the LDS tile (ksize 3: W > 2289). */
int gtts_conv_dgrad_small(const float *dy, const float *w, const float *mask, float *dx, int B, int cin, int cout, int H, int W,
                          int ksize, gtts_stream_t stream);
/* Gradient of gtts_diffusion_noising w.r.t. x0 and mu (z and z_masked carry none): dx0 = d mask dxt, dmu = (1 - d) mask dxt, with
 * d = e^{-cum/2} evaluated exactly as the forward kernel does.  dxt, dx0, dmu [B,F,T]; dx0 or dmu may be NULL, not both. */
int gtts_diffusion_noising_backward(const float *dxt, const float *mask, const float *t, float beta_min, float beta_max, float *dx0,
                                    float *dmu, int B, int F, int T, gtts_stream_t stream);
/* path [B,t_x,T]: the 0/1 alignment of monotonic_align.maximum_path (at most one 1 per column, a token's frames one contiguous run).
 * idx [B,T] int32: the token of each frame, -1 for an empty column; dur [B,t_x] fp32: frames per token (exact integers, what
 * path.sum(-1) gives); first [B,t_x] int32: the first frame of each token's run, -1 for a token without frames.  T <= 40960. */
int gtts_align_index(const float *path, int *idx, float *dur, int *first, int B, int t_x, int T, gtts_stream_t stream);
/* Duration loss (tts.py:141-143, utils.py:42-44) without its normaliser: partials[b] = sum_i (logw - log(1e-8 + dur) x_mask)[b,i]^2,
 * grad (nullable) [B,t_x] = 2 (logw - log(1e-8 + dur) x_mask); loss = sum(partials) / sum(x_lengths).  logw, dur, x_mask [B,t_x]. */
int gtts_duration_loss(const float *logw, const float *dur, const float *x_mask, float *partials, float *grad, int B, int t_x,
                       gtts_stream_t stream);
/* The training crop and the aligned prior mean in one gather (tts.py:146-172): output frame c of sample b is input frame start[b] + c
 * while c < kept[b] and empty from there on (no crop: S = T, start = 0, kept = y_lengths).
 *   y_c[b,f,c] = y[b,f,start+c],  mu_y[b,f,c] = mu_x[b,f,idx[b,start+c]] (0 where idx is -1); both 0 for c >= kept[b]
 *   partials[gtts_align_gather_partials(B,F,S)]: fixed-order sums of 0.5 ((y_c - mu_y)^2 + log 2 pi) over the live elements
 *   (prior loss = sum(partials) / (sum(kept) F), tts.py:178-180).
 * mu_x [B,F,t_x], y [B,F,T], idx [B,T], start / kept [B] int32 ON THE DEVICE (a kept[b] above S counts as S; start[b] + c is clamped
 * into [0, T - 1]); y_c, mu_y [B,F,S].  GTTS_E_SHAPE: B, F, t_x, T or S < 1, S > T (a window longer than the frame axis: every kept[b]
 * would lie below S, a batch the dense composition's own mask, sequence_mask(kept), cannot take either). */
size_t gtts_align_gather_partials(int B, int F, int S);
int gtts_align_gather_forward(const float *mu_x, const float *y, const int *idx, const int *start, const int *kept, float *y_c, float *mu_y,
                              float *partials, int B, int F, int t_x, int T, int S, gtts_stream_t stream);
/* Its gradient w.r.t. mu_x, a segment sum over each token's run (nothing is scattered):
 *   dmu_x[b,f,i] = sum over the live output frames c of token i, ascending c, of (g_mu_y[b,f,c] + scale[0] (mu_y - y_c)[b,f,c])
 * scale: ONE float on the device, (gradient of the prior loss) / (sum(kept) F); g_mu_y or scale may be NULL (not both; mu_y and y_c are
 * read only with scale).  Tokens without a live frame get 0.  dur, first as written by gtts_align_index; dmu_x [B,F,t_x]. */
int gtts_align_gather_backward(const float *g_mu_y, const float *mu_y, const float *y_c, const float *scale, const float *dur,
                               const int *first, const int *start, const int *kept, float *dmu_x, int B, int F, int t_x, int S,
                               gtts_stream_t stream);

/* ---- ABI 7 (additive): the condition path of the DiffVC decoder's training step (csrc/train_cond.hip, csrc/train_inglu.hip) -----------
 * All fp32 VALU kernels, no atomics, every sum in a fixed order: two calls on the same inputs give the same bits.  The caller owns
 * every buffer; arguments are checked on the host before anything is launched (GTTS_E_NULL, then GTTS_E_SHAPE: B, C, H, W < 1,
 * B > 65535 or H W >= 2^31, then GTTS_E_CONFIG).
 * Condition field: the convolution of the condition vector broadcast over the mel plane (DiffVC/model/diffusion.py:74-76) as the bias
 * field it is.  U [B,taps,C], taps = 9 in (kh, kw) order (a 3x3 convolution with padding 1) or 1 (a 1x1); mask [B,W]:
 *   out[b,c,h,w] = base[b,c,h,w] + sum_{kh,kw} [0 <= h+kh-1 < H][0 <= w+kw-1 < W] mask[b,w+kw-1] U[b,kh,kw,c]     (taps 1: mask[b,w] U[b,c])
 * base (nullable: zeros) and out [B,C,H,W], two buffers.  GTTS_E_CONFIG for any other taps. */
int gtts_cond_field_forward(const float *U, const float *mask, const float *base, float *out, int B, int C, int H, int W, int taps,
                            gtts_stream_t stream);
/* S[b,kh,kw,c] = sum_{h,w} dy[b,c,h,w] (the same gates): dy [B,C,H,W] is read once -> S [B,taps,C]. */
int gtts_cond_field_backward(const float *dy, const float *mask, float *S, int B, int C, int H, int W, int taps, gtts_stream_t stream);
/* RefBlock's masked mean (DiffVC/model/modules.py:165-166): p[b,c] = sum_{h,w} y[b,c,h,w] mask[b,w] / (sum_w mask[b,w] H), y [B,C,H,W],
 * mask [B,W] -> p [B,C] (a row of mask without a live column divides by zero, as the composition does), and its gradient
 * dy[b,c,h,w] = dp[b,c] mask[b,w] / (sum_w mask[b,w] H). */
int gtts_masked_mean_forward(const float *y, const float *mask, float *p, int B, int C, int H, int W, gtts_stream_t stream);
int gtts_masked_mean_backward(const float *dp, const float *mask, float *dy, int B, int C, int H, int W, gtts_stream_t stream);
/* gtts_in_glu_forward / _backward with RefBlock's time-bias add (modules.py:159,162) behind the GLU: out = IN-GLU(y) + tb[b,c], tb [B,C];
 * the backward call also writes dtb [B,C] = sum_{h,w} dout.  stats and scratch as for gtts_in_glu_*; dy, dgamma and dbeta have the bits
 * gtts_in_glu_backward gives on the same dout. */
int gtts_in_glu_tb_forward(const float *y, const float *gamma, const float *beta, const float *tb, float *out, float *stats, int B, int C,
                           int H, int W, float eps, gtts_stream_t stream);
int gtts_in_glu_tb_backward(const float *dout, const float *y, const float *gamma, const float *beta, const float *stats, float *dy,
                            float *dgamma, float *dbeta, float *dtb, float *scratch, int B, int C, int H, int W, gtts_stream_t stream);

/* RefBlock's narrow 3x3 convolutions (csrc/train_narrow.hip): cin 1 or 32, cout 64 or 128 (GTTS_E_CONFIG otherwise; the data gradient:
 * cin 32), padding 1, the semantics of gtts_conv3x3_masked --
 *   y[b,n,h,w] = omask[b,w] (bias[n] + sum_{k,kh,kw} w[n,k,kh,kw] x[b,k,h+kh-1,w+kw-1] mask[b,w+kw-1])      omask nullable (no output mask)
 * on the fp32-input MFMA (fp32 products, fp32 accumulation in a fixed order: fp32-grade results, the same bits on every call).
 * x [B,cin,H,W], w [cout][cin][3][3] (the module's layout, nothing packed by the caller), mask / omask [B,W], y / dy [B,cout,H,W].
 * workspace: gtts_conv3x3_narrow_workspace_bytes(B, cin, cout, H, W, op) bytes, op 0 forward, 1 data gradient (both: the re-laid-out
 * weights), 2 weight gradient (per-slice partial sums, added in slice order by a second kernel); 0 for what the entry points refuse.
 * GTTS_E_SHAPE: B, H, W < 1, B > 65535, H W >= 2^29; GTTS_E_WORKSPACE: fewer bytes than that.
 *   dgrad  dx = mask * (the convolution of dy omask with the transposed, flipped weights): the gradient of the forward call w.r.t. x
 *   wgrad  dw [cout][cin][3][3] and db [cout] (nullable) of the forward call: sums over (dy omask) and (x mask) */
size_t gtts_conv3x3_narrow_workspace_bytes(int B, int cin, int cout, int H, int W, int op);
int gtts_conv3x3_narrow_forward(const float *x, const float *mask, const float *omask, const float *w, const float *bias, float *y,
                                void *workspace, size_t workspace_bytes, int B, int cin, int cout, int H, int W, gtts_stream_t stream);
int gtts_conv3x3_narrow_dgrad(const float *dy, const float *omask, const float *mask, const float *w, float *dx, void *workspace,
                              size_t workspace_bytes, int B, int cin, int cout, int H, int W, gtts_stream_t stream);
int gtts_conv3x3_narrow_wgrad(const float *x, const float *mask, const float *omask, const float *dy, float *dw, float *db, void *workspace,
                              size_t workspace_bytes, int B, int cin, int cout, int H, int W, gtts_stream_t stream);

/* ---- debugging / tests: named intermediates of the last estimator call (keep_intermediates plans) ----- */
int gtts_plan_num_tensors(const gtts_plan *plan);
/* offset is in bytes into the workspace for the given (B,T); dims = {B,C,H,W}. */
int gtts_plan_tensor_info(const gtts_plan *plan, int i, int B, int T, const char **name, size_t *offset,
                          int dims[4]);
/* same for DiffVC plans, whose RefBlock tensors live on the reference mel's frame axis (T_ref) */
int gtts_vc_tensor_info(const gtts_plan *plan, int i, int B, int T, int T_ref, const char **name, size_t *offset,
                        int dims[4]);

/* ---- measurement: per-op HIP-event timing of the op program (bench.py roofline) ------------------------- */
/* Ops are the kernel launches of one estimator call, in launch order; label = layer name, kernel = the HIP kernel
 * (template instance) it launches, flops / bytes = ALGORITHMIC work of that launch for the given (B,T)
 * (SURVEY.md section 8d model: each tensor read once, written once). */
int gtts_plan_num_ops(const gtts_plan *plan);
int gtts_plan_op_info(const gtts_plan *plan, int i, int B, int T, const char **label, const char **kernel,
                      double *flops, double *bytes);
/* on != 0: every later estimator / sampler call brackets each op launch with hipEventRecord on the call's stream;
 * while profiling, the sampler runs the batch unsplit on that one stream (no sub-batch streams). */
int gtts_profile_enable(gtts_plan *plan, int on);
/* Synchronises the recorded events, adds elapsed milliseconds and launch counts per op into the two arrays
 * (length gtts_plan_num_ops) and clears the record. */
int gtts_profile_collect(gtts_plan *plan, double *ms_per_op, long long *launches_per_op);
/* ABI 4: gtts_profile_enable(plan, 2) keeps the sub-batch streams ON and brackets every launch with events on ITS stream;
 * gtts_profile_timeline then returns, per launch (at most cap), the op index, the stream (0: the call's stream, 1 + h: side
 * stream h) and start / end in milliseconds relative to the first recorded launch (HIP event timestamps share one clock
 * across streams): an un-traced timeline of which kernels were in flight together.  Clears the record. */
int gtts_profile_timeline(gtts_plan *plan, int cap, int *op, int *stream, double *t0_ms, double *t1_ms, int *n);

/* ---- measurement: ceilings of THIS chip, measured (SURVEY.md section 8d "a measured hipMemcpy/stream-triad ceiling") ----
 * Both enqueue ONE kernel on `stream`; the caller times it (HIP events) and divides.  Nothing on the sampling path calls them.
 * gtts_ubench_mfma: `workgroups` x 4 waves each issue iters x 8 independent v_mfma_f32_32x32x16_bf16 whose operand fragments
 *   are read from src (>= 4096 bytes of bf16 data: pass random values -- the chip clocks to its power budget and all-zero
 *   operands overstate what live data reaches); out: gtts_ubench_mfma_out_floats(workgroups) floats; *flops = FLOPs enqueued;
 *   iters < 0: |iters| sweeps of 16 independent v_mfma_f32_16x16x32_bf16 instead (the other bf16 shape).
 * gtts_ubench_hbm: mode 0 c = a (8 bytes per element), 1 c = a + 1.5 b (12), 2 read-only sweep of a (4), + 4: the same with
 *   nontemporal loads / stores; n floats, a multiple of 4, buffers 16-byte aligned; *bytes = bytes the launch moves. */
size_t gtts_ubench_mfma_out_floats(int workgroups);
int gtts_ubench_mfma(const void *src, size_t src_bytes, float *out, int workgroups, int iters, double *flops, gtts_stream_t stream);
int gtts_ubench_hbm(const float *a, const float *b, float *c, size_t n, int mode, int workgroups, double *bytes, gtts_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GRADTTS_ABI_H */
