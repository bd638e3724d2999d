"""Catalogue of single-op cases of the DiffVC decoder's condition path under training (csrc/train_cond.hip, the time-bias entries of
csrc/train_inglu.hip), with float64 references and float64 restatements of what the kernels compute.

  F  condition field     out = base + the convolution of a condition vector broadcast over the plane, as a bias field; S = d / d U
  P  masked mean         RefBlock's pooling, its broadcast backward, and the tail final_conv -> * mask -> mean with the pooling first
  G  InstanceNorm + GLU + time bias, forward and every gradient
  N  narrow 3x3 convolutions (cin 1 or 32): conv(x * mask) + bias [* output mask], weight + bias gradient, data gradient

  reference    float64 autograd of the torch composition (`*_composition`): F.conv2d of the mask plane with the per-sample field weights;
               the masked sum over the division; RefBlock's own tail; InstanceNorm2d -> GLU -> + tb; F.conv2d of the masked input.
               e_ref32 = the same autograd in fp32 torch on the CPU
  restatement  `*_manual`: the formulas of include/gradtts_abi.h in float64, with the mistakes of *_MISTAKES restated on them
  error        per tensor  e = max |got - ref64| / max |ref64|  (an all-zero reference asks for exact zeros)
  GPU bound    e <= 4 e_ref32 + 2e-6 and e <= 1e-4 (the project's per-op bound for fp32 kernels, tests/glue_train_cases.py); the
               integer-valued cases must be exact in every element
Shapes: every H in {1, 2, 3, 80} with every W in {1, 2, 3, 5, 67, 130} (no neighbour, one neighbour, both borders adjacent, an odd size,
more than one pass of 256 threads at H W > 256, the training height), B in {1, 3}, C in {64, 256}; masks all ones, ragged tails, one
sample of length 1, interior holes.  tests/test_cond_train_cases_cpu.py proves the restatements against the references and that the
bound tells every restated mistake from the contract."""
import collections
import itertools
import math

import torch
import torch.nn.functional as F

from case_util import relerr_zero_exact as relerr, seq_mask as _seq_mask  # noqa: F401

GRAD_ABS = 2e-6
GRAD_REL = 1e-4
HS, WS = (1, 2, 3, 80), (1, 2, 3, 5, 67, 130)
MASK_KINDS = ("ones", "ragged", "len1", "holes")


def bound(e32):
    return min(4.0 * e32 + GRAD_ABS, GRAD_REL)


def make_mask(kind, B, W):
    """[B, W] fp32 of 0 / 1.  ones; ragged: a full sample, one cut mid-row, one a column short; len1: the second sample (the only one at
    B = 1) keeps one column; holes: the ragged tails with every third interior column dead as well."""
    if kind == "ones":
        return torch.ones(B, W)
    if kind == "len1":
        return _seq_mask(([W, 1, W // 2 + 1] if B > 1 else [1])[:B], W)
    m = _seq_mask(([W, W // 2 + 1, max(1, W - 1)] if B > 1 else [W // 2 + 1])[:B], W)
    if kind == "holes":
        m[:, 1::3] = 0.0
        m[:, 0] = 1.0                       # (every sample keeps a live column: the pool divides by their number)
    return m


def _shapes():
    """(B, C, H, W, mask kind) for every H x W: B, C and the mask kind rotate; the two largest planes take the lighter (B, C) pairs."""
    out = []
    for i, (H, W) in enumerate(itertools.product(HS, WS)):
        B, C = (1, 3)[i % 2], (64, 256)[(i // 2) % 2]
        if H * W > 5000 and B * C > 256:
            B, C = (3, 64) if i % 2 else (1, 256)
        out.append((B, C, H, W, MASK_KINDS[(i + i // 6) % 4]))
    return out


# ============================================================================================================ F: the condition field
FCase = collections.namedtuple("FCase", "id B C H W mask taps base ints")
F_CASES = [FCase("field-b%d-c%d-%dx%d-%s-t%d%s" % (B, C, H, W, kind, taps, "" if base else "-nobase"), B, C, H, W, kind, taps, base, False)
           for j, (B, C, H, W, kind) in enumerate(_shapes()) for taps, base in ((9, j % 3 != 0), (1, j % 3 != 1))]
F_CASES += [FCase("field-int-b3-c64-%dx%d-holes-t%d" % (H, W, taps), 3, 64, H, W, "holes", taps, True, True)
            for H, W in ((3, 5), (80, 67)) for taps in (9, 1)]
F_BY_ID = {c.id: c for c in F_CASES}
F_MISTAKES = ("gate_on_own_column", "no_row_gate", "row_wrap")


def _leaf(t, dtype):
    """A fresh leaf of `dtype` holding t's values (the catalogue's inputs themselves never require a gradient)."""
    return t.detach().clone().to(dtype).requires_grad_(True)


def _draw(g, shape, ints):
    return torch.randint(-3, 4, shape, generator=g).float() if ints else torch.randn(shape, generator=g)


def f_inputs(c):
    g = torch.Generator().manual_seed(3000 + 7 * c.H + c.W + c.C + c.taps)
    return dict(U=_draw(g, (c.B, c.taps, c.C), c.ints), base=_draw(g, (c.B, c.C, c.H, c.W), c.ints) if c.base else None,
                dy=_draw(g, (c.B, c.C, c.H, c.W), c.ints), mask=make_mask(c.mask, c.B, c.W))


def f_composition(c, d, dtype=torch.float64):
    """out and S = d <out, dy> / d U by autograd through F.conv2d: per sample, the mask plane [1, 1, H, W] (the masked constant plane
    of value 1) convolved with the field's values as a [C, 1, k, k] weight, zero padding."""
    U = _leaf(d["U"], dtype)
    k = 3 if c.taps == 9 else 1
    rows = []
    for b in range(c.B):
        plane = d["mask"][b].to(dtype).expand(1, 1, c.H, c.W)
        rows.append(F.conv2d(plane, U[b].t().reshape(c.C, 1, k, k), None, padding=k // 2))
    out = torch.cat(rows, 0)
    if c.base:
        out = out + d["base"].to(dtype)
    out.backward(d["dy"].to(dtype))
    return dict(out=out.detach(), S=U.grad)


def _gates(c, d, mistake=None):
    """[B, taps, H, W] float64: the factor of U[b, tap] in out[b, :, h, w]."""
    m = d["mask"].double()
    if c.taps == 1:
        return m[:, None, None, :].expand(c.B, 1, c.H, c.W).clone()
    g = torch.zeros(c.B, 9, c.H, c.W, dtype=torch.float64)
    hs, ws = torch.arange(c.H), torch.arange(c.W)
    flat = F.pad(m.repeat(1, c.H), (1, 1))                                    # the mask over the flattened plane, for the wrap
    for kh in range(3):
        rows = torch.ones(c.H, dtype=torch.float64) if mistake == "no_row_gate" else ((hs + kh - 1 >= 0) & (hs + kh - 1 < c.H)).double()
        for kw in range(3):
            inside = ((ws + kw - 1 >= 0) & (ws + kw - 1 < c.W)).double()
            if mistake == "row_wrap":                                         # column w + kw - 1 of the flattened plane: the next row's end
                cols = flat[:, (hs[:, None] * c.W + ws[None, :] + kw).reshape(-1)].view(c.B, c.H, c.W)
                g[:, kh * 3 + kw] = cols * rows[None, :, None]
                continue
            cols = m * inside if mistake == "gate_on_own_column" else F.pad(m, (1, 1))[:, kw:kw + c.W]
            g[:, kh * 3 + kw] = rows[None, :, None] * cols[:, None, :]
    return g


def f_manual(c, d, mistake=None):
    g = _gates(c, d, mistake)
    out = torch.einsum("bthw,btc->bchw", g, d["U"].double())
    if c.base:
        out = out + d["base"].double()
    return dict(out=out, S=torch.einsum("bthw,bchw->btc", g, d["dy"].double()))


# ================================================================================================================ P: the masked mean
PCase = collections.namedtuple("PCase", "id B C H W mask ints")
P_CASES = [PCase("pool-b%d-c%d-%dx%d-%s" % s, *s, False) for s in _shapes()]
P_CASES += [PCase("pool-int-b3-c64-%dx%d-holes" % (H, W), 3, 64, H, W, "holes", True) for H, W in ((3, 5), (80, 67))]
P_BY_ID = {c.id: c for c in P_CASES}
P_MISTAKES = ("no_H", "bias_lost")
P_COUT = 8                                  # output channels of the tail's 1x1 weight in the composition


def p_inputs(c):
    g = torch.Generator().manual_seed(4000 + 7 * c.H + c.W + c.C)
    return dict(y=_draw(g, (c.B, c.C, c.H, c.W), c.ints) + (0.0 if c.ints else 0.5), dp=_draw(g, (c.B, c.C), c.ints),
                mask=make_mask(c.mask, c.B, c.W), wf=torch.randn(P_COUT, c.C, 1, 1, generator=g) / math.sqrt(c.C),
                bf=torch.randn(P_COUT, generator=g) + 1.0)


def p_composition(c, d, dtype=torch.float64):
    """p and dy = d <p, dp> / d y by autograd of RefBlock.forward's pooling, (y * mask).sum((2, 3)) / (mask.sum((2, 3)) * H); `tail`:
    its last two lines as they stand, final_conv(y * mask) -> * mask -> that mean."""
    y = _leaf(d["y"], dtype)
    m = d["mask"].to(dtype)[:, None, None, :]
    p = (y * m).sum((2, 3)) / (m.sum((2, 3)) * c.H)
    p.backward(d["dp"].to(dtype))
    with torch.no_grad():
        z = F.conv2d(y * m, d["wf"].to(dtype), d["bf"].to(dtype))
        tail = (z * m).sum((2, 3)) / (m.sum((2, 3)) * c.H)
    return dict(p=p.detach(), dy=y.grad, tail=tail.detach())


def p_manual(c, d, mistake=None):
    """p[b,c] = sum_{h,w} y m / (sum_w m H), dy = dp m / (sum_w m H); tail = p Wf^T + bf (the mean of a constant is the constant)."""
    m = d["mask"].double()
    den = m.sum(1) * (1.0 if mistake == "no_H" else float(c.H))
    p = torch.einsum("bchw,bw->bc", d["y"].double(), m) / den[:, None]
    dy = (d["dp"].double() / den[:, None])[:, :, None, None] * m[:, None, None, :].expand(c.B, 1, c.H, c.W)
    tail = p @ d["wf"].double().view(P_COUT, c.C).t()
    if mistake != "bias_lost":
        tail = tail + d["bf"].double()
    return dict(p=p, dy=dy, tail=tail)


# ============================================================================================= G: InstanceNorm + GLU + time bias
GCase = collections.namedtuple("GCase", "id B C H W")
G_CASES = [GCase("inglu-tb-b%d-c%d-%dx%d" % s, *s) for s in ((3, 32, 80, 20), (2, 64, 3, 5), (1, 64, 2, 67), (2, 32, 17, 130))]
G_BY_ID = {c.id: c for c in G_CASES}
G_MISTAKES = ("tb_before_glu",)
G_EPS = 1e-5
G_TENSORS = ("out", "dy", "dgamma", "dbeta", "dtb")


def g_inputs(c):
    g = torch.Generator().manual_seed(5000 + c.W + c.C)
    return dict(y=torch.randn(c.B, 2 * c.C, c.H, c.W, generator=g) * 2.0 + 0.3, gamma=1.0 + 0.3 * torch.randn(2 * c.C, generator=g),
                beta=0.2 * torch.randn(2 * c.C, generator=g), tb=torch.randn(c.B, c.C, generator=g), dout=torch.randn(c.B, c.C, c.H, c.W, generator=g))


def g_composition(c, d, dtype=torch.float64, mistake=None):
    """InstanceNorm2d(affine) -> GLU(dim=1) -> + tb[:, :, None, None] (DiffVC/model/modules.py:152-162) under autograd."""
    y, gamma, beta, tb = (_leaf(d[n], dtype) for n in ("y", "gamma", "beta", "tb"))
    n = F.instance_norm(y, None, None, gamma, beta, True, 0.0, G_EPS)
    if mistake == "tb_before_glu":
        n = torch.cat((n[:, :c.C] + tb[:, :, None, None], n[:, c.C:]), 1)
        out = F.glu(n, 1)
    else:
        out = F.glu(n, 1) + tb[:, :, None, None]
    out.backward(d["dout"].to(dtype))
    return dict(out=out.detach(), dy=y.grad, dgamma=gamma.grad, dbeta=beta.grad, dtb=tb.grad)


def g_manual(c, d, mistake=None):
    """The kernel's own formulas in float64: statistics per (sample, channel) plane, biased variance; d tb = sum over the plane of d out."""
    y, gamma, beta, tb, dout = (d[n].double() for n in ("y", "gamma", "beta", "tb", "dout"))
    mean, var = y.mean((2, 3), keepdim=True), y.var((2, 3), unbiased=False, keepdim=True)
    xh = (y - mean) / torch.sqrt(var + G_EPS)
    n = xh * gamma[None, :, None, None] + beta[None, :, None, None]
    a, sg = n[:, :c.C], torch.sigmoid(n[:, c.C:])
    if mistake == "tb_before_glu":
        a = a + tb[:, :, None, None]
    out = a * sg + (0.0 if mistake == "tb_before_glu" else tb[:, :, None, None])
    dn = torch.cat((dout * sg, dout * a * sg * (1.0 - sg)), 1)
    dgamma, dbeta = (dn * xh).sum((0, 2, 3)), dn.sum((0, 2, 3))
    dxh = dn * gamma[None, :, None, None]
    dy = (dxh - dxh.mean((2, 3), keepdim=True) - xh * (dxh * xh).mean((2, 3), keepdim=True)) / torch.sqrt(var + G_EPS)
    dtb = (dout * sg).sum((2, 3)) if mistake == "tb_before_glu" else dout.sum((2, 3))
    return dict(out=out, dy=dy, dgamma=dgamma, dbeta=dbeta, dtb=dtb)


# ============================================================================================================ N: narrow convolutions
NCase = collections.namedtuple("NCase", "id B cin cout H W omask")
N_CASES = [NCase("narrow-c%d-o%d-%dx%d%s" % (ci, co, H, W, "-om" if om else ""), 2, ci, co, H, W, om)
           for ci, co in ((1, 64), (32, 64), (32, 128)) for (H, W), om in (((1, 1), False), ((3, 5), True), ((17, 130), False), ((80, 36), True))]
N_BY_ID = {c.id: c for c in N_CASES}


def n_inputs(c):
    g = torch.Generator().manual_seed(6000 + c.cin + c.cout + c.W)
    dy = torch.randn(c.B, c.cout, c.H, c.W, generator=g)
    for sl in ((..., 0, slice(None)), (..., -1, slice(None)), (..., slice(None), 0), (..., slice(None), -1)):
        dy[sl] *= 4.0
    return dict(x=torch.randn(c.B, c.cin, c.H, c.W, generator=g), w=torch.randn(c.cout, c.cin, 3, 3, generator=g) / math.sqrt(c.cin * 9),
                bias=torch.randn(c.cout, generator=g), dy=dy, mask=make_mask("ragged", c.B, c.W))


def n_composition(c, d, dtype=torch.float64):
    """y = conv2d(x * mask, w, bias, padding 1) [* mask] and dw, db, dx by autograd."""
    x, w, bias = (_leaf(d[n], dtype) for n in ("x", "w", "bias"))
    m = d["mask"].to(dtype)[:, None, None, :]
    y = F.conv2d(x * m, w, bias, padding=1)
    if c.omask:
        y = y * m
    y.backward(d["dy"].to(dtype))
    return dict(y=y.detach(), dw=w.grad, db=bias.grad, dx=x.grad)
