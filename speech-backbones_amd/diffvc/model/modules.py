"""Building blocks of the DiffVC decoder (DiffVC/model/modules.py).  Lines 16-110 of the reference are byte-identical
to Grad-TTS's blocks, so those classes are shared; SinusoidalPosEmb hard-codes the 1000x scale (modules.py:123) and
RefBlock (modules.py:128-166) is specific to DiffVC."""
import math

import torch

from ...model.base import BaseModule
from ...model.diffusion import (Block, Downsample, LinearAttention, Mish, Residual, ResnetBlock, Rezero,  # noqa: F401
                                Upsample)


class SinusoidalPosEmb(BaseModule):
    """modules.py:113-125."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, x):
        half = self.dim // 2
        freq = torch.exp(torch.arange(half, device=x.device).float() * -(math.log(10000) / (half - 1)))
        arg = 1000.0 * x[:, None] * freq[None, :]
        return torch.cat((arg.sin(), arg.cos()), dim=-1)


def _conv_in_glu(cin, cout):
    return torch.nn.Sequential(torch.nn.Conv2d(cin, cout, 3, 1, 1), torch.nn.InstanceNorm2d(cout, affine=True),
                               torch.nn.GLU(dim=1))


class RefBlock(BaseModule):
    """Reference-mel summariser: 6 x (conv3x3 -> InstanceNorm -> GLU) with two time-bias adds, 1x1 conv, masked mean."""

    def __init__(self, out_dim, time_emb_dim):
        super().__init__()
        base = out_dim // 4
        self.mlp1 = torch.nn.Sequential(Mish(), torch.nn.Linear(time_emb_dim, base))
        self.mlp2 = torch.nn.Sequential(Mish(), torch.nn.Linear(time_emb_dim, 2 * base))
        self.block11 = _conv_in_glu(1, 2 * base)
        self.block12 = _conv_in_glu(base, 2 * base)
        self.block21 = _conv_in_glu(base, 4 * base)
        self.block22 = _conv_in_glu(2 * base, 4 * base)
        self.block31 = _conv_in_glu(2 * base, 8 * base)
        self.block32 = _conv_in_glu(4 * base, 8 * base)
        self.final_conv = torch.nn.Conv2d(4 * base, out_dim, 1)

    @staticmethod
    def _block(blk, y, mask, tb=None):
        """conv3x3(y * mask) -> InstanceNorm -> GLU [+ tb[:, :, None, None]] (DiffVC/model/modules.py:140-162).  Training on the GPU: the
        convolution (forward, data and weight gradient) on the gtts:: training kernels where their tiles allow (64 or a multiple of 128
        channels on both sides: block22 / block31 / block32 = 90 % of RefBlock's FLOPs at out_dim 128; the narrow layer kinds listed in
        _train_ops.COND_LEFT_ON_TORCH stay on the framework's convolution), InstanceNorm + GLU of all six blocks on csrc/train_inglu.hip,
        with the time-bias add of block12 / block22 and its gradient inside those kernels."""
        from ...model import _train_ops as T
        from ...model._backend import backend
        conv, norm = blk[0], blk[1]
        if not (torch.is_grad_enabled() and T._hip(y) and y.dim() == 4):
            h = blk(y * mask)
            return h if tb is None else h + tb[:, :, None, None]
        be, kind = backend(), (conv.in_channels, conv.out_channels)
        narrow = be.conv3x3_narrow(*kind)
        if (kind not in T.COND_LEFT_ON_TORCH and conv.kernel_size == (3, 3) and
                be.conv3x3_supported(*kind, need_dgrad=y.requires_grad or not narrow, shape=(y.shape[0], y.shape[2], y.shape[3]))):
            T._count(True)
            if narrow:
                T.cond_count(True)
            h = T.MaskedConv3x3.apply(y.contiguous(), mask, conv.weight, conv.bias, None)
        else:
            T.cond_count(False)
            h = conv(y * mask)
        if norm.affine and not norm.track_running_stats:
            T._count(True)
            if tb is not None:
                T.cond_count(True)
            return T.InstNormGlu.apply(h.contiguous(), norm.weight, norm.bias, norm.eps, None if tb is None else tb.contiguous())
        h = blk[2](norm(h))
        if tb is not None:
            T.cond_count(False)
            h = h + tb[:, :, None, None]
        return h

    def forward(self, x, mask, time_emb):
        """modules.py:152-166.  Training on the GPU: final_conv -> * mask -> masked mean is linear, so the plane is pooled first
        (csrc/train_cond.hip) and the 1x1 weight is applied to the pooled [B, 4 base] vector; the bias passes through the mean
        unchanged."""
        from ...model import _train_ops as T
        y = self._block(self.block12, self._block(self.block11, x, mask), mask, self.mlp1(time_emb))
        y = self._block(self.block22, self._block(self.block21, y, mask), mask, self.mlp2(time_emb))
        y = self._block(self.block32, self._block(self.block31, y, mask), mask)
        fc = self.final_conv
        if torch.is_grad_enabled() and T._hip(y) and T._hip(mask) and fc.kernel_size == (1, 1):
            T.cond_count(True)
            p = T.MaskedMean.apply(y.contiguous(), mask)
            return torch.nn.functional.linear(p, fc.weight.view(fc.out_channels, fc.in_channels), fc.bias)
        y = self.final_conv(y * mask)
        return (y * mask).sum((2, 3)) / (mask.sum((2, 3)) * x.shape[2])
