"""Autograd composition of the score U-Net -- TRAINING ONLY (the sampling path under torch.no_grad never comes here).

Training (Diffusion.compute_loss -> loss_t -> estimator with autograd, Grad-TTS/model/diffusion.py:281-294) needs gradients
w.r.t. the same nn.Parameters.  On HIP tensors every tensor-sized op of the network runs on the hand-written kernels of
csrc/train*.hip behind torch.autograd.Function wrappers:
  MaskedConv3x3        Block's 3x3 convolution (forward / data gradient on the inference MFMA kernel, weight gradient as a
                       wave-specialised MFMA reduction over pixels); the up path's torch.cat is read in place (two sources)
  GnMishMask           GroupNorm + Mish + mask (+ ResnetBlock's time term), forward and backward fused
  MaskedConv7x7        DiffVC PostNet Block's 7x7 convolution (forward / data gradient on the inference CONV_C7 kernel, weight
                       gradient on train_wgrad7.hip); PostNetInitConv / PostNetFinalConv its single-channel 1x1 convolutions (postnet())
  MaskedConv1x1        res_conv, to_qkv, to_out (forward / data gradient on the CONV_P1 kernel, MFMA weight gradient)
  LinearAttentionCore  softmax over pixels, context, output (forward and backward)
  RezeroResidual, MaskedResidualAdd, the plain residual add, FinalConv (64 -> 1 with both masks), ScoreLoss
  ResampleConv         Downsample / Upsample forward and all their gradients on the HIP kernels (Downsample's data gradient is an
                       Upsample call, Upsample's gradients are 3x3 stride-1 operations over the four stride-2 phases of dy)
  Noising, DurationLoss, AlignGather   what couples encoder and decoder in GradTTS.compute_loss (the train.py step): the noising with its
                       gradient w.r.t. the prior mean, and the alignment glue between MAS and the decoder -- frames per token and the
                       duration loss, the training crop, mu_y = attn^T . mu_x and the prior loss -- as index / gather / segment-sum
                       kernels of csrc/glue_train.hip; the first layer's data gradient (the stacked (mu, xt[, spk]) planes carry a
                       gradient then) is gtts_conv_dgrad_small, taken by MaskedConv3x3 / MaskedConv1x1 for 2 or 3 input planes
  EncAttentionCore     the transformer encoder's windowed relative-position attention between its convolutions, and EncLayerNorm, its
                       LayerNorm with the fused residual (text_encoder.py, shared by TextEncoder and DiffVC's MelEncoder), on
                       csrc/enc_train.hip
  EncConv1d            the encoders' Conv1d layers (prenet, attention projections, FFN, proj_m, duration predictor, MelEncoder's
                       init_proj / term_proj) with their masks: data gradient on the inference kernel of csrc/conv1d.h, weight / bias
                       gradient on csrc/conv1d_train.hip, forward on that kernel too or (as wired: ENC_CONV_KERNEL_FORWARD) torch's
                       fp32 conv1d; ReLU, dropout, residual adds and the embedding stay torch autograd
  MaskedMean, InstNormGlu (tb), CondField   the condition path of the DiffVC decoder (csrc/train_cond.hip, train_inglu.hip): RefBlock's
                       tail pooled before its 1x1 weight, its time-bias adds inside InstanceNorm + GLU; RefBlock's narrow 3x3 layers
                       (cin 1 / 32) go through MaskedConv3x3 to the fp32-MFMA kernels of csrc/train_narrow.hip; CondField, a condition
                       vector's convolution over the plane as a bias field, is an op with its tests that the step does not use
The [B, dim] time / speaker MLPs stay stock torch ops.  On CPU tensors (tests) everything is stock torch.
"""
import math

import torch
import torch.nn.functional as F

from ._backend import backend


FORCE_TORCH = False      # measurement switch (bench.py train_step): route every op to stock PyTorch-ROCm kernels


def _hip(t):
    """THE gate: an fp32 HIP tensor while the kernels are not switched off (FORCE_TORCH is read at call time: bench.py and the tools
    assign it on this module) -- what every training kernel takes."""
    return not FORCE_TORCH and t.is_cuda and t.dtype == torch.float32


enc_hip = _hip           # (the encoder modules' name for it)


def _cols(mask):
    """A mask's [B,W] view ([B,1,1,W], or PostNet's [B,1,W]; no copy of a contiguous mask); None stays None."""
    return None if mask is None else mask.reshape(mask.shape[0], mask.shape[-1])


class _OpCounter:
    """One (hip_ops, torch_fallback_ops) pair: how many ops of one part of the training path ran on the gtts:: kernels and how many
    fell back to stock torch ops.  Nothing is counted while FORCE_TORCH is on."""
    __slots__ = ("hip_ops", "torch_fallback_ops")

    def __init__(self):
        self.reset()

    def reset(self):
        self.hip_ops = self.torch_fallback_ops = 0

    def read(self):
        return self.hip_ops, self.torch_fallback_ops

    def count(self, hip, n=1):
        if not FORCE_TORCH:
            if hip:
                self.hip_ops += n
            else:
                self.torch_fallback_ops += n


# How many tensor-sized ops of the training path ran on the gtts:: kernels and how many fell back to stock torch ops because a gate
# (shape, dtype, device, channel multiple) failed.  A fallback is correct but slow, and silent otherwise: callers / tests read
# `op_counts()` after a step (tests/test_gpu_training.py asserts (n, 0) on the reference's shapes).
_COUNTS = _OpCounter()
reset_op_counts, op_counts, _count = _COUNTS.reset, _COUNTS.read, _COUNTS.count

# The same pair for the transformer encoder's two kernel ops (EncAttentionCore, EncLayerNorm: text_encoder.py counts one per call
# made with autograd on -- `hip` when the kernels of csrc/enc_train.hip ran, `fallback` when the module's torch composition did).
# A pair of its own: op_counts() keeps counting the decoder / PostNet ops only.
_ENC_COUNTS = _OpCounter()
reset_enc_op_counts, enc_op_counts, enc_count = _ENC_COUNTS.reset, _ENC_COUNTS.read, _ENC_COUNTS.count

# And for the alignment glue of GradTTS.compute_loss (model/tts.py): one count per op -- the path's index form, the duration loss, the
# crop / prior-mean gather with the prior loss -- `hip` when the kernels of csrc/glue_train.hip ran, `fallback` when HIP tensors took
# the dense torch composition.
_GLUE_COUNTS = _OpCounter()
reset_glue_op_counts, glue_op_counts, glue_count = _GLUE_COUNTS.reset, _GLUE_COUNTS.read, _GLUE_COUNTS.count

# And for the condition path of the DiffVC decoder (RefBlock's narrow convolutions, its two time-bias adds and its pooled tail; the two
# condition fields where a caller uses them): one count per op -- `hip` when the kernels of csrc/train_cond.hip / train_inglu.hip ran,
# `fallback` when HIP tensors took stock torch ops.  A GradLogPEstimator with use_ref_t counts 6 ops per step: 3 narrow convolutions,
# 2 time-bias adds, 1 pool; the fallbacks are the narrow convolutions of COND_LEFT_ON_TORCH.
_COND_COUNTS = _OpCounter()
reset_cond_op_counts, cond_op_counts, cond_count = _COND_COUNTS.reset, _COND_COUNTS.read, _COND_COUNTS.count

# And for the encoders' Conv1d layers (enc_conv1d below: prenet, attention projections, FFN, proj_m, duration predictor, MelEncoder's
# init_proj / term_proj): one count per convolution called with autograd on -- `hip` when EncConv1d ran, `fallback` when the module call did.
_ENC_CONV_COUNTS = _OpCounter()
reset_enc_conv_op_counts, enc_conv_op_counts, enc_conv_count = _ENC_CONV_COUNTS.reset, _ENC_CONV_COUNTS.read, _ENC_CONV_COUNTS.count


class MaskedConv3x3(torch.autograd.Function):
    """y = Conv2d_3x3(cat(x, x1) * mask) + bias with all three gradients on the HIP kernels (x1 None: one source)."""

    @staticmethod
    def forward(ctx, x, mask, weight, bias, x1=None):
        be = backend()
        cols = _cols(mask)
        ctx.save_for_backward(x, cols, weight, x1)
        return be.conv3x3_masked(x, cols, weight, bias, x1)

    @staticmethod
    def backward(ctx, dy):
        be = backend()
        x, cols, weight, x1 = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dx1 = dw = db = None
        need1 = x1 is not None and ctx.needs_input_grad[4]
        if ctx.needs_input_grad[0] or need1:
            c0 = x.shape[1]
            if x1 is None and c0 in (2, 3):                         # first layer (stacked planes): its own kernel, one pass over dy
                dx = be.conv_dgrad_small(dy, weight, cols)
            elif x1 is None:
                dx = be.conv3x3_dgrad(dy, weight, cols)             # (the mask rides in the convolution's epilogue)
            else:                                                   # mask and split in one pass each (contiguous results)
                full = be.conv3x3_dgrad(dy, weight)
                if ctx.needs_input_grad[0]:
                    dx = be.add_masked(None, full, cols, channels=(0, c0))
                if need1:
                    dx1 = be.add_masked(None, full, cols, channels=(c0, full.shape[1]))
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:      # (one kernel produces both)
            dw, db = be.conv3x3_wgrad(x, cols, dy, x1)
        return dx, None, (dw if ctx.needs_input_grad[2] else None), (db if ctx.needs_input_grad[3] else None), dx1


class MaskedConv7x7(torch.autograd.Function):
    """y = Conv2d_7x7(x * mask, padding 3) + bias (DiffVC PostNet Block, DiffVC/model/postnet.py:21-23) with all three gradients on
    the HIP kernels: forward and data gradient on the inference CONV_C7 kernel, weight / bias gradient on csrc/train_wgrad7.hip."""

    @staticmethod
    def forward(ctx, x, mask, weight, bias):
        be = backend()
        cols = _cols(mask)
        ctx.save_for_backward(x, cols, weight)
        return be.conv7x7_masked(x, cols, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        be = backend()
        x, cols, weight = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = be.conv7x7_dgrad(dy, weight, cols)                 # (the mask rides in the convolution's epilogue)
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:      # (one kernel produces both)
            dw, db = be.conv7x7_wgrad(x, cols, dy)
        return dx, None, (dw if ctx.needs_input_grad[2] else None), (db if ctx.needs_input_grad[3] else None)


class MaskedConv1x1(torch.autograd.Function):
    """y = Conv2d_1x1(x * mask) + bias (res_conv, to_qkv, to_out: diffusion.py:70,87-88; mask and bias optional) with all three
    gradients on the HIP kernels.  A 1x1 convolution does not mix columns, so the mask of the data gradient is applied to dy
    by the same kernel prologue."""

    @staticmethod
    def forward(ctx, x, mask, weight, bias):
        be = backend()
        cols = _cols(mask)
        ctx.save_for_backward(x, cols, weight)
        ctx.has_bias = bias is not None
        return be.conv1x1_masked(x, cols, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        be = backend()
        x, cols, weight = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = be.conv_dgrad_small(dy, weight, cols) if x.shape[1] in (2, 3) else be.conv1x1_dgrad(dy, weight, cols)
        if ctx.needs_input_grad[2] or (ctx.has_bias and ctx.needs_input_grad[3]):
            dw, db = be.conv1x1_wgrad(x, cols, dy, want_bias=ctx.has_bias)
        return dx, None, (dw if ctx.needs_input_grad[2] else None), (db if ctx.has_bias and ctx.needs_input_grad[3] else None)


class LinearAttentionCore(torch.autograd.Function):
    """softmax over pixels of k, context = k~ v^T, out = context^T q (LinearAttention.forward between its two 1x1 convolutions,
    diffusion.py:90-100) on to_qkv's output [B, 384, H, W]; forward and backward on csrc/train_attn.hip."""

    @staticmethod
    def forward(ctx, qkv):
        out, c, stat = backend().attn_train_forward(qkv)
        ctx.save_for_backward(qkv, c, stat)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, c, stat = ctx.saved_tensors
        return backend().attn_train_backward(qkv, dout.contiguous(), c, stat)


class RezeroResidual(torch.autograd.Function):
    """f * g + x (Residual(Rezero(fn)), diffusion.py:40-46,103-108) with d f = dy * g, d g = sum(dy * f), d x = dy."""

    @staticmethod
    def forward(ctx, f, g, x):
        ctx.save_for_backward(f, g)
        return backend().rezero_forward(f, g, x)

    @staticmethod
    def backward(ctx, dy):
        f, g = ctx.saved_tensors
        dy = dy.contiguous()
        df, dg = backend().rezero_backward(dy, f, g)
        return df, dg, dy


class GnMishMask(torch.autograd.Function):
    """Mish(GroupNorm(y)) * mask (Block.forward, diffusion.py:53-58) [+ tb[:, :, None, None]: ResnetBlock's time term,
    diffusion.py:75-76] with forward and backward on the HIP kernels."""

    @staticmethod
    def forward(ctx, y, mask, gamma, beta, groups, eps, tb=None):
        be = backend()
        cols = _cols(mask)
        out, stats = be.gn_mish_forward(y, gamma, beta, cols, groups, eps, tb)
        ctx.save_for_backward(y, cols, gamma, beta, stats)
        ctx.groups = groups
        ctx.has_tb = tb is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        y, cols, gamma, beta, stats = ctx.saved_tensors
        r = backend().gn_mish_backward(dout.contiguous(), y, gamma, beta, cols, stats, ctx.groups, want_dtb=ctx.has_tb)
        return r[0], None, r[1], r[2], None, None, (r[3] if ctx.has_tb else None)


class InstNormGlu(torch.autograd.Function):
    """InstanceNorm2d(affine) -> GLU(dim=1) on a convolution output [B, 2C, H, W] (DiffVC RefBlock, DiffVC/model/modules.py:128-157)
    [+ tb[:, :, None, None]: RefBlock's time-bias adds, modules.py:159,162 -- the add rides in the kernel's store and its gradient, a sum
    over the plane, in the backward kernel's reduction] with forward and backward on csrc/train_inglu.hip."""

    @staticmethod
    def forward(ctx, y, gamma, beta, eps, tb=None):
        out, stats = backend().in_glu_forward(y, gamma, beta, eps, tb)
        ctx.save_for_backward(y, gamma, beta, stats)
        ctx.has_tb = tb is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        y, gamma, beta, stats = ctx.saved_tensors
        r = backend().in_glu_backward(dout.contiguous(), y, gamma, beta, stats, want_dtb=ctx.has_tb)
        return r[0], r[1], r[2], None, (r[3] if ctx.has_tb else None)


class CondField(torch.autograd.Function):
    """base + the convolution of a condition vector broadcast over the mel plane, as the bias field it is (csrc/train_cond.hip): U
    [B, taps, C] = the weight's condition columns contracted with the vector (taps 9: 3x3 in (kh, kw) order, 1: 1x1), mask [B,1,1,W].
    d U is the gated sum of dy over the plane, d base is dy."""

    @staticmethod
    def forward(ctx, U, mask, base):
        cols = _cols(mask)
        ctx.save_for_backward(cols)
        ctx.taps = U.shape[1]
        return backend().cond_field(U, cols, base.shape[2], base)

    @staticmethod
    def backward(ctx, dy):
        (cols,) = ctx.saved_tensors
        dy = dy.contiguous()
        dU = backend().cond_field_backward(dy, cols, ctx.taps) if ctx.needs_input_grad[0] else None
        return dU, None, (dy if ctx.needs_input_grad[2] else None)


class MaskedMean(torch.autograd.Function):
    """(y * mask).sum((2, 3)) / (mask.sum((2, 3)) * H) (RefBlock's pooling, DiffVC/model/modules.py:165-166): y [B,C,H,W] -> [B,C]."""

    @staticmethod
    def forward(ctx, y, mask):
        cols = _cols(mask)
        ctx.save_for_backward(cols)
        ctx.H = y.shape[2]
        return backend().masked_mean(y, cols)

    @staticmethod
    def backward(ctx, dp):
        (cols,) = ctx.saved_tensors
        return backend().masked_mean_backward(dp.contiguous(), cols, ctx.H), None


class MaskedResidualAdd(torch.autograd.Function):
    """h + v * mask (ResnetBlock with an identity res_conv, diffusion.py:77-78; mask None: h + v)."""

    @staticmethod
    def forward(ctx, h, v, mask):
        cols = _cols(mask)
        ctx.save_for_backward(cols)
        return backend().add_masked(h, v, cols)

    @staticmethod
    def backward(ctx, dout):
        (cols,) = ctx.saved_tensors
        dout = dout.contiguous()
        dv = dout if cols is None else (backend().add_masked(None, dout, cols) if ctx.needs_input_grad[1] else None)
        return dout, dv, None


class FinalConv(torch.autograd.Function):
    """(final_conv(x * mask)) * mask for the 64 -> 1 convolution (diffusion.py:175-176)."""

    @staticmethod
    def forward(ctx, x, mask, weight, bias):
        cols = _cols(mask)
        ctx.save_for_backward(x, cols, weight)
        return backend().final_conv_forward(x, weight, bias, cols)

    @staticmethod
    def backward(ctx, dout):
        x, cols, weight = ctx.saved_tensors
        dx, dw, db = backend().final_conv_backward(x, weight, cols, dout.contiguous())
        return dx, None, dw, db


class PostNetInitConv(torch.autograd.Function):
    """init_conv(x * mask) for PostNet's 1 -> C 1x1 convolution (DiffVC/model/postnet.py:43,49-51): x [B,F,T] -> [B,C,F,T].  The bias
    lands on masked frames too, as in the reference (every consumer multiplies by the mask again)."""

    @staticmethod
    def forward(ctx, x, cols, weight, bias):
        ctx.save_for_backward(x, cols, weight)
        return backend().postnet_expand(x, cols, weight.reshape(-1), bias)

    @staticmethod
    def backward(ctx, dout):
        be = backend()
        x, cols, weight = ctx.saved_tensors
        dout = dout.contiguous()
        dx = be.postnet_collapse(dout, cols, weight.reshape(-1)) if ctx.needs_input_grad[0] else None
        dw, db = be.postnet_chan_dot(dout, x, cols)
        return dx, None, dw.reshape(weight.shape), db


class PostNetFinalConv(torch.autograd.Function):
    """final_conv(x * mask) for PostNet's C -> 1 1x1 convolution (DiffVC/model/postnet.py:45,53): [B,C,F,T] -> [B,F,T], NO output
    mask (unlike the decoder's FinalConv)."""

    @staticmethod
    def forward(ctx, x, cols, weight, bias):
        ctx.save_for_backward(x, cols, weight)
        return backend().postnet_collapse(x, cols, weight.reshape(-1), bias)

    @staticmethod
    def backward(ctx, dout):
        be = backend()
        x, cols, weight = ctx.saved_tensors
        dout = dout.contiguous()
        dx = be.postnet_expand(dout, cols, weight.reshape(-1)) if ctx.needs_input_grad[0] else None
        dw, _ = be.postnet_chan_dot(x, dout, cols, want_sum=False)
        _, db = be.postnet_chan_dot(dout.unsqueeze(1), None, None, want_dot=False)
        return dx, None, dw.reshape(weight.shape), db


class ResampleConv(torch.autograd.Function):
    """Downsample / Upsample of x * mask (diffusion.py:19-34,158,171): forward on the inference kernels; Downsample's data
    gradient is an Upsample call with the zero-padded kernel and its weight gradient the stride-1 MFMA reduction against the
    zero-inserted dy; Upsample's gradients are the 3x3 convolution / weight gradient over the four stride-2 phases of dy."""

    @staticmethod
    def forward(ctx, x, mask, weight, bias, up):
        cols = _cols(mask)
        ctx.save_for_backward(x, cols, weight)
        ctx.up = bool(up)
        ctx.bias_n = int(bias.shape[0])
        return backend().conv_resample(x, cols, weight, bias, up)

    @staticmethod
    def backward(ctx, dy):
        be = backend()
        x, cols, weight = ctx.saved_tensors
        dy = dy.contiguous()
        need_dx = ctx.needs_input_grad[0]
        if not ctx.up:
            # stride 2: the weight gradient is the stride-1 one against the zero-inserted dy (MFMA reduction of train_wgrad.hip)
            gw, gb = be.conv3x3_wgrad(x, cols, be.zero_insert2(dy))
            gi = None
            if need_dx:
                ones = be._const(dy.device, "ones", int(dy.shape[0]), int(dy.shape[3]))
                gi = be.conv_resample(dy, ones, weight, None, True, dgrad_of_down=True)
        else:
            # ConvTranspose2d 4x4 stride 2 pad 1: output row oy = 2 iy - 1 + ky.  Over the four stride-2 phases of dy (even / odd
            # rows x columns, stacked as channels) both gradients are stride-1 3x3 operations: odd rows meet taps ky = 0, 2 at
            # offsets -1, 0; even rows taps ky = 1, 3 at offsets 0, +1 (the same for columns).
            P = be.space_to_depth2(dy)                              # [B, 4 cout, h, w], block (pr * 2 + pc), pr = 1: even rows
            ci, co = int(weight.shape[0]), int(weight.shape[1])
            tap = _up_tap_index(dy.device)                          # [2 (phase), 3 (ky')] -> ky, 4 = no tap
            ones = be._const(dy.device, "ones", int(dy.shape[0]), int(x.shape[3]))
            gi = None
            if need_dx:
                wz = torch.cat((weight.reshape(ci, co, 4, 4), weight.new_zeros(ci, co, 1, 4)), dim=2)
                wz = torch.cat((wz, wz.new_zeros(ci, co, 5, 1)), dim=3)                        # [ci, co, 5, 5], index 4 = zero
                wp = wz[:, :, tap[:, None, :, None], tap[None, :, None, :]]                    # [ci, co, pr, pc, ky', kx']
                wp = wp.permute(0, 2, 3, 1, 4, 5).reshape(ci, 4 * co, 3, 3).contiguous()
                gi = be.conv3x3_masked(P, ones, wp, be._const(dy.device, "zeros", ci))
            xm = be.add_masked(None, x, cols)
            d6, _ = be.conv3x3_wgrad(P, ones, xm)                   # [ci][4 co][3][3]: "dy" role = x * mask, "x" role = the phases
            d6 = d6.reshape(ci, 2, 2, co, 3, 3)
            pr, kp = _up_tap_inverse(dy.device)                     # ky -> (phase, ky')
            gw = d6[:, pr[:, None], pr[None, :], :, kp[:, None], kp[None, :]].permute(2, 3, 0, 1).contiguous()
            gb = dy.sum((0, 2, 3))
        dx = be.add_masked(None, gi, cols) if need_dx else None
        return dx, None, gw, gb, None


_UP_IDX = {}


def _up_tap_index(device):
    """[phase (0 odd rows, 1 even rows)][ky' of the 3x3 view] -> ky of the 4x4 kernel, 4 where the phase has no tap."""
    key = (str(device), "fwd")
    if key not in _UP_IDX:
        _UP_IDX[key] = torch.tensor([[0, 2, 4], [4, 1, 3]], dtype=torch.long, device=device)
    return _UP_IDX[key]


def _up_tap_inverse(device):
    """ky of the 4x4 kernel -> (phase, ky' of the 3x3 view)."""
    key = (str(device), "inv")
    if key not in _UP_IDX:
        _UP_IDX[key] = (torch.tensor([0, 1, 0, 1], dtype=torch.long, device=device), torch.tensor([0, 1, 1, 2], dtype=torch.long, device=device))
    return _UP_IDX[key]


class ScoreLoss(torch.autograd.Function):
    """sum((eps * sqrt(1 - e^{-cum}) + z)^2) / denom with the gradient produced in the same pass (diffusion.py:285-287)."""

    @staticmethod
    def forward(ctx, eps, z, t, beta_min, beta_max, inv_denom):
        loss, g = backend().score_loss(eps, z, t, beta_min, beta_max, inv_denom, want_grad=True)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (g,) = ctx.saved_tensors
        return g * dloss, None, None, None, None, None


class Noising(torch.autograd.Function):
    """Diffusion.forward_diffusion given the N(0,1) draw z, under autograd (GradTTS.compute_loss: mu comes from the encoder): the forward
    is gtts_diffusion_noising -- the bits of the decoder-only path --, the backward gtts_diffusion_noising_backward.  z and the second
    output (z * mask) carry no gradient."""

    @staticmethod
    def forward(ctx, x0, mu, z, mask, t, beta_min, beta_max):
        xt, zm = backend().diffusion_noising(x0, mu, z, mask, t, beta_min, beta_max)
        ctx.save_for_backward(mask, t)
        ctx.betas = (beta_min, beta_max)
        ctx.mark_non_differentiable(zm)
        return xt, zm

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dxt, _dzm):
        mask, t = ctx.saved_tensors
        dx0, dmu = backend().diffusion_noising_backward(dxt.contiguous(), mask, t, ctx.betas[0], ctx.betas[1],
                                                        want_dx0=ctx.needs_input_grad[0], want_dmu=ctx.needs_input_grad[1])
        return dx0, dmu, None, None, None, None, None


class DurationLoss(torch.autograd.Function):
    """sum((logw - log(1e-8 + dur) * x_mask)^2) * inv_denom (tts.py:141-143, utils.py:42-44) with the gradient w.r.t. logw produced in
    the same pass; dur: frames per token (align_index), inv_denom: 1 / sum(x_lengths) as a device scalar."""

    @staticmethod
    def forward(ctx, logw, dur, x_mask, inv_denom):
        total, g = backend().duration_loss(logw, dur, x_mask, want_grad=True)
        ctx.save_for_backward(g, inv_denom)
        return total * inv_denom

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dloss):
        g, inv_denom = ctx.saved_tensors
        return g * (dloss * inv_denom), None, None, None


class AlignGather(torch.autograd.Function):
    """The training crop of y and of the alignment, mu_y = attn^T . mu_x and the prior loss (tts.py:146-181) as one gather:
    (y_c, mu_y, prior_loss) from mu_x, y and the index form of the path (align_index).  Output frame c of sample b is input frame
    start[b] + c while c < kept[b]; inv_denom: 1 / (sum(kept) * n_feats) as a device scalar.  The backward is a segment sum over each
    token's run of frames: the gradient arriving through mu_y (the decoder) plus the prior loss's own."""

    @staticmethod
    def forward(ctx, mu_x, y, idx, dur, first, start, kept, S, inv_denom):
        y_c, mu_y, total = backend().align_gather(mu_x, y, idx, start, kept, S)
        ctx.save_for_backward(mu_y, y_c, dur, first, start, kept, inv_denom)
        ctx.mark_non_differentiable(y_c)
        ctx.set_materialize_grads(False)
        return y_c, mu_y, total * inv_denom

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _dy_c, g_mu_y, g_prior):
        mu_y, y_c, dur, first, start, kept, inv_denom = ctx.saved_tensors
        if g_mu_y is None and g_prior is None:
            return (None,) * 9
        scale = None if g_prior is None else (g_prior * inv_denom).reshape(1)
        dmu_x = backend().align_gather_backward(None if g_mu_y is None else g_mu_y.contiguous(), mu_y, y_c, scale, dur, first, start, kept)
        return (dmu_x,) + (None,) * 8


# RefBlock's narrow 3x3 convolutions, as (cin, cout), that run on the framework's convolution under autograd; every other convolution
# of the condition path runs on the gtts:: kernels.  RefBlock.final_conv and the condition columns of the first ResnetBlock are never
# listed: the first is no convolution any more (MaskedMean), the second runs on the trunk's MFMA kernels.  tests/test_gpu_cond_train_modules.py records the step's
# torch.nn.functional.conv2d calls against this set.
# Left on torch by measurement (tools/vc_cond_train_step.py --layers on an MI355X, B = 16 x 80 x 128, forward + every gradient of one
# layer, median of 9): the fp32-MFMA kernels of csrc/train_narrow.hip take 0.44 ms (1 -> 64), 1.00 ms (32 -> 64) and 1.72 ms (32 -> 128)
# against 0.23, 0.36 and 0.58 ms of the framework's convolution.  The kernels stay, with their per-op tests (they are fp32-exact and
# repeat bit for bit); a kind leaves this set when its kernel is the faster one.
COND_LEFT_ON_TORCH = frozenset({(1, 64), (32, 64), (32, 128)})


class EncAttentionCore(torch.autograd.Function):
    """MultiHeadAttention.attention between its convolutions (text_encoder.py:145-175), self-attention with relative embeddings shared
    by the heads, forward (dropout multiplier `drop` [b, h, t, t] or None) and backward on csrc/enc_train.hip.  Saved: the inputs and
    `stat` [b, h, t, 2] (row maximum, reciprocal row sum) -- the backward recomputes the probabilities from them."""

    @staticmethod
    def forward(ctx, q, k, v, cols, ek, ev, drop, n_heads, window):
        be = backend()
        ek2 = None if ek is None else ek.detach().reshape(ek.shape[-2], ek.shape[-1]).contiguous()
        ev2 = None if ev is None else ev.detach().reshape(ev.shape[-2], ev.shape[-1]).contiguous()
        out, stat = be.enc_attention_train_forward(q, k, v, cols, ek2, ev2, drop, n_heads=n_heads, window=window)
        ctx.save_for_backward(q, k, v, cols, ek2, ev2, drop, stat)
        ctx.n_heads, ctx.window = n_heads, window
        ctx.rel_shape = None if ek is None else tuple(ek.shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        q, k, v, cols, ek, ev, drop, stat = ctx.saved_tensors
        dq, dk, dv, dek, dev = backend().enc_attention_train_backward(q, k, v, cols, ek, ev, drop, stat, dout.contiguous(),
                                                                      n_heads=ctx.n_heads, window=ctx.window)
        if dek is not None:
            dek, dev = dek.reshape(ctx.rel_shape), dev.reshape(ctx.rel_shape)
        return dq, dk, dv, None, dek, dev, None, None, None


class EncLayerNorm(torch.autograd.Function):
    """LayerNorm over channels of a [+ bres] (text_encoder.py:12-27): forward on the inference kernel (gtts_enc_layernorm), backward on
    csrc/enc_train.hip, which recomputes mean and rstd from the saved inputs."""

    @staticmethod
    def forward(ctx, a, gamma, beta, bres, eps):
        ctx.save_for_backward(a, gamma, beta, bres)
        ctx.eps = eps
        return backend().enc_layernorm(a, gamma.detach(), beta.detach(), bres=bres, eps=eps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        a, gamma, beta, bres = ctx.saved_tensors
        da, dbres, dgamma, dbeta = backend().enc_layernorm_backward(dout.contiguous(), a, gamma.detach(), beta.detach(), bres=bres,
                                                                    eps=ctx.eps)
        return da, dgamma, dbeta, dbres, None


_ENC_CONV_HANDLES = {}     # (cin, cout, K, dilation) -> (forward handle, transposed handle), or None where the kernel refuses the geometry


def _enc_conv_handles(cin, cout, K, dilation):
    """Host metadata only, made once per geometry: the layer's handle and the channel-swapped one its data gradient runs on."""
    key = (int(cin), int(cout), int(K), int(dilation))
    if key not in _ENC_CONV_HANDLES:
        be = backend()
        try:
            _ENC_CONV_HANDLES[key] = (be.Conv1dOp(0, cin, cout, K, dilation), be.Conv1dOp(0, cout, cin, K, dilation))
        except RuntimeError:       # more taps or a wider halo than the kernel holds (gtts_conv1d_create): the module call serves it
            _ENC_CONV_HANDLES[key] = None
    return _ENC_CONV_HANDLES[key]


# Which forward enc_conv1d gives EncConv1d.  The encoders' gradients are far more sensitive to the forward's rounding than to the
# backward's: on the GradTTS fixture of tests/test_gpu_tts_train_path.py a forward error of the split-bf16 grade (1.5e-6 of each
# convolution's largest output, emulated on the CPU) moves ~100 parameter gradients by 1e-3 ... 1.7e-3 -- and, where it flips the sign of
# one ReLU input, a whole row of an FFN weight gradient by 0.17 -- against that test's 5e-4, while the same error on every gradient the
# convolutions return moves none by more than 2.8e-5.  So the wiring keeps the module's own fp32 convolution in the
# forward and takes the kernels for the backward; EncConv1d(..., kernel_forward=True) is the all-kernel form, with the inference bits.
ENC_CONV_KERNEL_FORWARD = False


# Layer geometries (cin, cout, K) whose kernel path measured SLOWER than torch.nn.Conv1d autograd at both training shapes -- B = 16,
# L = 190 (train.py) and B = 128, L = 128 (train_enc.py); tools/enc_conv_train_prof.py, profiles/enc_conv_train.json, the numbers in
# DESIGN section 4.6.5 -- are left on the module call by enc_conv1d and counted as fallbacks.  Of the reference's nine layer kinds only
# DurationPredictor.conv_2 (256 -> 256, k = 3: faster at the train.py shape) is not among them; the kernels are a first version and are
# not tuned in this change.  Geometries nobody measured (other widths) take the kernels.
ENC_CONV_LEFT_ON_TORCH = frozenset({(192, 192, 5), (192, 192, 1), (192, 768, 3), (768, 192, 3), (192, 80, 1), (80, 192, 1), (192, 256, 3),
                                    (256, 1, 1)})


class EncConv1d(torch.autograd.Function):
    """y = (Conv1d(x * in_mask) + bias) * out_mask for a stride-1 'same'-padded Conv1d (masks [B, L] or None).  Backward: the data
    gradient on the inference kernel (csrc/conv1d.h) with the weight packed transposed and tap-reversed, the weight / bias gradient on
    csrc/conv1d_train.hip.  Forward: with kernel_forward the inference kernel (gtts_conv1d_forward: the bits of that layer in
    gtts_enc_forward), else torch's conv1d on x * in_mask -- the bits of the module call.  The packed copies are made here, on the
    stream, and live for this forward + backward; nothing synchronises and no random number is drawn."""

    @staticmethod
    def forward(ctx, x, weight, bias, in_mask, out_mask, dilation=1, kernel_forward=True):
        be = backend()
        cout, cin, K = weight.shape
        ctx.save_for_backward(x, weight, in_mask, out_mask)
        ctx.dilation, ctx.has_bias = dilation, bias is not None
        if not kernel_forward:
            y = F.conv1d(x if in_mask is None else x * in_mask.unsqueeze(1), weight, bias, padding=dilation * (K - 1) // 2, dilation=dilation)
            return y if out_mask is None else y * out_mask.unsqueeze(1)
        fwd, _ = _enc_conv_handles(cin, cout, K, dilation)
        b = be._const(x.device, "zeros", cout) if bias is None else bias.detach().contiguous()
        return fwd.forward(fwd.pack_into(weight.detach().contiguous()), b, x, in_mask=in_mask, out_mask=out_mask)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        be = backend()
        x, weight, in_mask, out_mask = ctx.saved_tensors
        cout, cin, K = weight.shape
        fwd, tr = _enc_conv_handles(cin, cout, K, ctx.dilation)
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:       # (false for MelEncoder.init_proj on a mel, the duration predictor's detached input)
            blob = tr.pack_dgrad(weight.detach().contiguous())
            dx = tr.forward(blob, be._const(x.device, "zeros", cin), dy, in_mask=out_mask, out_mask=in_mask)
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_db:      # (one kernel produces both)
            dw, db = fwd.wgrad(x, dy, in_mask, out_mask, want_bias=want_db)
        return dx, (dw if ctx.needs_input_grad[1] else None), db, None, None, None, None


def _enc_conv_mask(m, B, L):
    """The [B, L] view of a sequence mask the kernels can take ([B, 1, L] or [B, L] fp32 on the device, no gradient), else None."""
    if not enc_hip(m) or m.requires_grad or m.numel() != B * L or m.shape[0] != B or m.shape[-1] != L:
        return None
    return m.reshape(B, L).contiguous()


def enc_conv1d(conv, x, in_mask=None, out_mask=None):
    """conv(x * in_mask) * out_mask for a Conv1d of the encoders (either mask may be None).  With autograd on, fp32 HIP tensors and a
    stride-1, ungrouped, zero-padded torch.nn.Conv1d with odd K and padding = dilation (K - 1) / 2 it runs EncConv1d, the masks riding in
    the kernels (forward: ENC_CONV_KERNEL_FORWARD); everything else -- CPU tensors, FORCE_TORCH, no_grad, any other geometry, a layer
    kind that measured slower than torch (ENC_CONV_LEFT_ON_TORCH) -- is the module call as written."""
    if torch.is_grad_enabled():
        args = _enc_conv_args(conv, x, in_mask, out_mask)
        enc_conv_count(args is not None)
        if args is not None:
            return EncConv1d.apply(*args)
    if in_mask is not None:
        x = x * in_mask
    y = conv(x)
    return y if out_mask is None else y * out_mask


def _enc_conv_args(conv, x, in_mask, out_mask):
    """EncConv1d's arguments when the kernels serve this call, else None."""
    if not (enc_hip(x) and x.dim() == 3 and type(conv) is torch.nn.Conv1d and enc_hip(conv.weight)):
        return None
    K, dil = conv.kernel_size[0], conv.dilation[0]
    if not (conv.stride == (1,) and conv.groups == 1 and conv.padding_mode == "zeros" and K % 2 == 1 and
            conv.padding == (dil * (K - 1) // 2,) and x.shape[1] == conv.in_channels and x.shape[0] >= 1 and x.shape[2] >= 1):
        return None
    if conv._forward_hooks or conv._forward_pre_hooks or (conv.bias is not None and not enc_hip(conv.bias)):
        return None
    B, cin, L = x.shape
    if (cin, conv.out_channels, K) in ENC_CONV_LEFT_ON_TORCH:
        return None
    # (a sample beyond the kernels' 32-bit byte offsets takes the module call up front instead of failing inside backward())
    if max((cin + 15) // 16 * 16, conv.out_channels) * L * 4 >= 2 ** 31 or _enc_conv_handles(cin, conv.out_channels, K, dil) is None:
        return None
    im = om = None
    if in_mask is not None:
        im = _enc_conv_mask(in_mask, B, L)
        if im is None:
            return None
    if out_mask is not None:
        om = _enc_conv_mask(out_mask, B, L)
        if om is None:
            return None
    return x.contiguous(), conv.weight, conv.bias, im, om, dil, ENC_CONV_KERNEL_FORWARD


def _block_conv_kind(conv):
    """Which training kernel family a Block's convolution belongs to: "3x3" (Grad-TTS / DiffVC decoder Blocks), "7x7" (DiffVC PostNet
    Blocks: 7x7, padding 3, stride 1 -- what the CONV_C7 kernels compute), or None (no kernel: stock torch)."""
    if conv.kernel_size == (3, 3):
        return "3x3"
    if conv.kernel_size == (7, 7) and conv.padding == (3, 3) and conv.stride == (1, 1) and conv.dilation == (1, 1):
        return "7x7"
    return None


def _hip_conv_ok(v, conv):
    # (shape: the kernels address one call's tensors with 32-bit byte offsets -- oversize batches / crops take the torch path
    # up front instead of failing inside loss.backward())
    if not _hip(v):
        return False
    shape = (v.shape[0], v.shape[2], v.shape[3])
    kind = _block_conv_kind(conv)
    if kind == "3x3":
        return backend().conv3x3_supported(conv.in_channels, conv.out_channels, need_dgrad=v.requires_grad, shape=shape)
    if kind == "7x7":
        return backend().conv7x7_supported(conv.in_channels, conv.out_channels, need_dgrad=v.requires_grad, shape=shape)
    return False


def _conv1x1(v, m, conv):
    """conv(v * m) for a 1x1 nn.Conv2d (m None: no mask)."""
    if (_hip(v) and conv.kernel_size == (1, 1) and
            backend().conv1x1_supported(conv.in_channels, conv.out_channels, need_dgrad=v.requires_grad,
                                        shape=(v.shape[0], v.shape[2], v.shape[3]))):
        _count(True)
        return MaskedConv1x1.apply(v.contiguous(), m, conv.weight, conv.bias)
    _count(False)
    return F.conv2d(v if m is None else v * m, conv.weight, conv.bias)


def _mish(v):
    return v * torch.tanh(F.softplus(v))


def _conv_gn_mish(blk, v, m, tb=None, v1=None):
    """Block.forward [+ the time term tb[:, :, None, None]] on v (or on the concatenation cat(v, v1), read in place)."""
    conv, norm = blk.block[0], blk.block[1]
    if v1 is not None and not (_hip_conv_ok(v, conv) and conv.kernel_size == (3, 3) and v.shape[1] % 64 == 0):
        v, v1 = torch.cat((v, v1), dim=1), None
    if _hip_conv_ok(v, conv):
        _count(True)
        if conv.kernel_size == (7, 7):
            y = MaskedConv7x7.apply(v.contiguous(), m, conv.weight, conv.bias)
        else:
            y = MaskedConv3x3.apply(v.contiguous(), m, conv.weight, conv.bias, None if v1 is None else v1.contiguous())
    else:
        _count(False)
        y = F.conv2d(v * m, conv.weight, conv.bias, padding=conv.padding)
    if _hip(y) and y.dim() == 4 and y.shape[1] % norm.num_groups == 0:
        _count(True)
        return GnMishMask.apply(y.contiguous(), m, norm.weight, norm.bias, norm.num_groups, norm.eps,
                                None if tb is None else tb.contiguous())
    _count(False)
    y = F.group_norm(y, norm.num_groups, norm.weight, norm.bias, norm.eps)
    y = _mish(y) * m
    return y if tb is None else y + tb[:, :, None, None]


def time_terms(blocks, temb):
    """ResnetBlock.mlp (Mish -> Linear, diffusion.py:66-67,75) of every block in one pass: Mish(temb) once, one Linear over the
    concatenated weights; returns the per-block [B, dim_out] terms (views).  The 12 blocks share the same input, and 36 separate
    [16 x 64] GEMMs and 80 elementwise launches cost more than the attention layers."""
    mt = _mish(temb)
    lins = [rb.mlp[1] for rb in blocks]
    tb = F.linear(mt, torch.cat([l.weight for l in lins], dim=0), torch.cat([l.bias for l in lins], dim=0))
    return list(torch.split(tb, [l.out_features for l in lins], dim=1))


def resnet(rb, v, m, temb, v1=None, tb=None):
    """ResnetBlock.forward (diffusion.py:73-78) on v, or on cat(v, v1) without materialising it.  tb: the block's time term if the
    caller has computed it (time_terms)."""
    if tb is None:
        lin = rb.mlp[1]
        tb = F.linear(_mish(temb), lin.weight, lin.bias)
    h = _conv_gn_mish(rb.block1, v, m, tb=tb, v1=v1)
    h = _conv_gn_mish(rb.block2, h, m)
    if isinstance(rb.res_conv, torch.nn.Conv2d):
        rc = rb.res_conv
        if v1 is None:
            r = _conv1x1(v, m, rc)
        elif _hip(v) and backend().conv1x1_supported(v.shape[1], rc.out_channels) and backend().conv1x1_supported(v1.shape[1], rc.out_channels):
            # a 1x1 convolution of a concatenation is the sum of the convolutions of its parts with the weight's column blocks
            c0 = v.shape[1]
            _count(True)
            r = MaskedConv1x1.apply(v.contiguous(), m, rc.weight[:, :c0].contiguous(), rc.bias)
            r = MaskedResidualAdd.apply(r, MaskedConv1x1.apply(v1.contiguous(), m, rc.weight[:, c0:].contiguous(), None), None)
        else:
            _count(False)
            r = F.conv2d(torch.cat((v, v1), dim=1) * m, rc.weight, rc.bias)
        return MaskedResidualAdd.apply(h, r.contiguous(), None) if _hip(h) else h + r
    if v1 is not None:
        v = torch.cat((v, v1), dim=1)
    return MaskedResidualAdd.apply(h, v.contiguous(), m) if _hip(h) else h + v * m


def _resample(v, m, conv, up):
    if _hip(v) and backend().resample_supported(v.shape[1], conv.out_channels, v.shape[2], v.shape[3], up, B=v.shape[0]):
        return ResampleConv.apply(v.contiguous(), m, conv.weight, conv.bias, up)
    return conv(v * m)


def attention(res, v):
    rez = res.fn
    att = rez.fn
    b, c, hh, ww = v.shape
    qkv = _conv1x1(v, None, att.to_qkv)
    hip = _hip(v) and att.heads == 4 and qkv.shape[1] == 384 and v.numel() % 4 == 0
    if hip:
        out = LinearAttentionCore.apply(qkv.contiguous())
    else:
        q, k, val = qkv.view(b, 3, att.heads, -1, hh * ww).unbind(1)
        k = torch.softmax(k, dim=-1)
        ctx = torch.matmul(k, val.transpose(-1, -2))            # [b, heads, d, e]
        out = torch.matmul(ctx.transpose(-1, -2), q)            # [b, heads, e, n]
        out = out.reshape(b, -1, hh, ww)
    y = _conv1x1(out, None, att.to_out)
    if hip:
        return RezeroResidual.apply(y.contiguous(), rez.g, v.contiguous())
    return y * rez.g + v


def time_embedding(est, t):
    half = est.dim // 2
    freq = torch.exp(torch.arange(half, device=t.device).float() * -(math.log(10000) / (half - 1)))
    arg = est.pe_scale * t[:, None] * freq[None, :]
    emb = torch.cat((arg.sin(), arg.cos()), dim=-1)
    l0, l2 = est.mlp[0], est.mlp[2]
    return F.linear(_mish(F.linear(emb, l0.weight, l0.bias)), l2.weight, l2.bias)


def _pack_specs(est):
    """Every convolution weight the HIP training kernels of one step multiply with, in the forms they need (forward packing and,
    where a data gradient is taken, the transposed one): the argument of backend().prepack.  First layers (2 / 3 stacked input
    planes) and Upsample's re-indexed gradient weight pack themselves where they are used."""
    be = backend()
    cached = est.__dict__.get("_gtts_pack_specs")
    if cached is not None and all(m.weight is s[0] for m, s in zip(cached.mods, cached)):
        return cached                                     # (the module tree is static; a Parameter that was REPLACED rebuilds the list)
    specs = be.PackSpecs()
    specs.mods = []
    for mod in est.modules():
        n0 = len(specs)
        if isinstance(mod, torch.nn.ConvTranspose2d):
            ci, co = mod.in_channels, mod.out_channels
            if mod.kernel_size == (4, 4) and be.resample_supported(ci, co, 2, 2, True):
                specs.append((mod.weight, ci, co, False, "up"))
        elif isinstance(mod, torch.nn.Conv2d):
            ci, co = mod.in_channels, mod.out_channels
            if mod.kernel_size == (3, 3) and mod.stride == (2, 2):
                if be.resample_supported(ci, co, 2, 2, False):
                    specs.append((mod.weight, ci, co, False, "dn"))
                    specs.append((mod.weight, co, ci, False, "dn_T"))
            elif mod.kernel_size == (3, 3) and mod.stride == (1, 1) and ci >= 16:
                if be.conv3x3_supported(ci, co, need_dgrad=True) and not be.conv3x3_narrow(ci, co):      # (the narrow kernels pack nothing)
                    specs.append((mod.weight, ci, co, False, "3x3"))
                    specs.append((mod.weight, co, ci, True, "3x3"))
            elif mod.kernel_size == (1, 1) and ci >= 16:
                if be.conv1x1_supported(ci, co, need_dgrad=True):
                    specs.append((mod.weight, ci, co, False, "1x1"))
                    specs.append((mod.weight, co, ci, True, "1x1"))
        specs.mods.extend([mod] * (len(specs) - n0))
    est.__dict__["_gtts_pack_specs"] = specs
    return specs


def estimator(est, x, mask, mu, t, spk=None):
    if not FORCE_TORCH and x.is_cuda:
        be = backend()
        be.new_pack_generation()               # packed weight copies live for this call's forward + backward only ...
        be.prepack(_pack_specs(est))           # ... and all of them are made here, in one launch (also under no_grad: a validation
                                               # call would otherwise pack ~45 weights one by one, each with its own allocation)
    temb = time_embedding(est, t)
    planes = [mu, x]
    if est.n_spks >= 2:
        l0, l2 = est.spk_mlp[0], est.spk_mlp[2]
        s = F.linear(_mish(F.linear(spk, l0.weight, l0.bias)), l2.weight, l2.bias)
        planes.append(s[:, :, None].expand(-1, -1, x.shape[-1]))
    v = torch.stack(planes, 1)
    m = mask[:, None]
    blocks = [rb for r1, r2, _, _ in est.downs for rb in (r1, r2)] + [est.mid_block1, est.mid_block2] + \
             [rb for r1, r2, _, _ in est.ups for rb in (r1, r2)]
    tbs = iter(time_terms(blocks, temb))
    skips, pyramid = [], [m]
    for r1, r2, att, down in est.downs:
        m = pyramid[-1]
        v = resnet(r1, v, m, temb, tb=next(tbs))
        v = attention(att, resnet(r2, v, m, temb, tb=next(tbs)))
        skips.append(v)
        if not isinstance(down, torch.nn.Identity):
            v = _resample(v, m, down.conv, False)
        pyramid.append(m[..., ::2].contiguous())        # (contiguous: every op below takes its [B, W] view without a copy)
    pyramid.pop()
    m = pyramid[-1]
    v = resnet(est.mid_block1, v, m, temb, tb=next(tbs))
    v = resnet(est.mid_block2, attention(est.mid_attn, v), m, temb, tb=next(tbs))
    for r1, r2, att, up in est.ups:
        m = pyramid.pop()
        v = resnet(r1, v, m, temb, v1=skips.pop(), tb=next(tbs))       # (torch.cat read in place)
        v = attention(att, resnet(r2, v, m, temb, tb=next(tbs)))
        v = _resample(v, m, up.conv, True)
    m = mask[:, None]
    v = _conv_gn_mish(est.final_block, v, m)
    return final_conv(est.final_conv, v, m)


def final_conv(fc, v, m):
    """final_conv(v * mask) * mask, squeezed (diffusion.py:214-216; DiffVC/model/diffusion.py:104-106)."""
    if _hip(v) and fc.out_channels == 1:
        _count(True)
        return FinalConv.apply(v.contiguous(), m, fc.weight, fc.bias).squeeze(1)
    _count(False)
    out = F.conv2d(v * m, fc.weight, fc.bias)
    return (out * m).squeeze(1)


def postnet(pn, x, mask):
    """PostNet.forward (DiffVC/model/postnet.py:47-53) with autograd on HIP tensors: x [B, n_feats, T], mask [B, 1, T] -> [B, n_feats, T].
    The same module tree as the stock path, every tensor-sized op on the gtts:: kernels: init_conv / final_conv on the single-channel
    kernels of csrc/postnet.hip, the two Blocks as MaskedConv7x7 + GnMishMask, res as MaskedConv1x1.  The gradient w.r.t. x flows
    back to the caller (the MelEncoder)."""
    if not FORCE_TORCH and x.is_cuda:
        backend().new_pack_generation()      # (packed copies of the weights live for this forward + backward only)
    m = mask.unsqueeze(1)                                           # [B,1,1,T]
    ic, fc = pn.init_conv, pn.final_conv
    hip_io = _hip(x) and mask.dtype == torch.float32 and ic.in_channels == 1 and fc.out_channels == 1
    cols = _cols(mask).contiguous() if hip_io else None
    if hip_io:
        _count(True)
        v = PostNetInitConv.apply(x.contiguous(), cols, ic.weight, ic.bias)
    else:
        _count(False)
        v = F.conv2d(x.unsqueeze(1) * m, ic.weight, ic.bias)
    rb = pn.res_block
    h = _conv_gn_mish(rb.block1, v, m)
    h = _conv_gn_mish(rb.block2, h, m)
    r = _conv1x1(v, m, rb.res)
    h = MaskedResidualAdd.apply(h, r.contiguous(), None) if _hip(h) and _hip(r) else h + r
    if hip_io:
        _count(True)
        return PostNetFinalConv.apply(h.contiguous(), cols, fc.weight, fc.bias)
    _count(False)
    return F.conv2d(h * m, fc.weight, fc.bias).squeeze(1)
