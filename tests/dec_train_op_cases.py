"""Catalogue of single-op cases of the decoder's training kernels that are no convolution (csrc/train_norm.hip, train_inglu.hip,
train_attn.hip and the noising / loss head of train.hip), with float64 references and float64 restatements of what the kernels compute.

  GN   GroupNorm + Mish + mask (+ time term)   _lib.gn_mish_forward / gn_mish_backward        Grad-TTS/model/diffusion.py:53-58, :75-76
  IN   InstanceNorm2d + GLU                    _lib.in_glu_forward / in_glu_backward          DiffVC/model/modules.py:128-157
  AT   LinearAttention core                    _lib.attn_train_forward / attn_train_backward  diffusion.py:90-100
  RZ   Rezero residual                         _lib.rezero_forward / rezero_backward          diffusion.py:40-46, :103-108
  NZ   noising and score-loss head             _lib.diffusion_noising / score_loss            diffusion.py:244-252, :281-288

  reference    float64 autograd of the plain torch expression (`*_reference`); e_ref32 = the same in fp32 torch on the CPU
  restatement  `*_manual`: the formulas the kernels' headers state, in float64, with the mistakes of `*_MISTAKES` restated on them
  error        per tensor  e = max |got - ref64| / max |ref64|  (an all-zero reference asks for exact zeros), except
                 means       |got - ref| / max |y|           (a mean near zero is no scale)
                 rstd, 1/S   max |got / ref - 1|             (element-wise relative)
                 dk          |got - ref| / max(max |ref|, max |k~ t|):  dk = k~ (t - r) is a cancelling difference (at N = 1 it is exactly
                             zero) -- the scale of Rezero.g in tests/test_gpu_training.py, applied to both terms of the difference
                 dg, random  |got - ref| / (|dy| |f|) <= 1e-5, the Cauchy-Schwarz rule of tests/test_gpu_training.py; with dy = |f| nothing
                             cancels and dg is held like every other tensor
  GPU bound    e <= 4 e_ref32 + 2e-6 and e <= cap: 1e-5 for forward outputs (the project's fp32 forward bound), 1e-4 for gradients
  caps on e_ref32 (E32_CAP, per family and data kind, asserted by tests/test_dec_train_op_cases_cpu.py; about twice the measured maximum)

Data kinds of the two norms: `plain` 2 randn + 0.3; `offset30` 30 + randn; `offset40` 30 + 0.75 randn; `offset300` 30 + 0.1 randn -- a
plane whose mean is 300 times its spread, where E[x^2] - mean^2 from fp32 sums cancels; `short` bias_c + randn * mask, a masked batch's
convolution output; `saturated` gamma * 15 (InstanceNorm: the gate half's), so Mish sees both tails and the clamp at 40 and the sigmoid
saturates.  Masks are ragged: one full utterance, then one of length 1.

Narrowed kinds.  `offset300`: fp32 torch itself is up to 1.3e-5 off on out (both norms) and, for GroupNorm, 2.0e-5 on dy, 1.7e-5 on
dbeta and 9.3e-5 on dgamma there (its mean, and x * scale + shift at 300, round at 1e-5 of the spread) -- within a factor 8 of the hard
caps, which leaves no room for a cap on e_ref32 with headroom whose fourfold stays under the bound: the case would stand or fall with
the reference.  Held at 300 : 1 is what does not pass through x_hat -- the statistics, whose fp32 reference is 1e-7 off, and dtb -- and
InstanceNorm's three gradients (fp32 reference at most 8e-6); the rest is printed.  Every tensor is held on `offset40`, where
4 e_ref32 stays under both caps with room (out 1.5e-6, dgamma 1.2e-5).
At the clamp t = 1e-5 the module's own expression 1 - exp(-cum) keeps three digits in fp32 (cum = 5e-7 against an ulp of
6e-8): sqrt(1 - e^{-cum}) is 2.4 % off in stock fp32 torch and in the kernel alike, which alone is 1.3e-5 of max |xt| on an N(0,1) draw --
above the forward cap, so the case would fail on the fp32 reference.  The cases keep t = 1e-5 and draw z ~ 0.1 N(0,1) on that sample
(e_ref32 <= 1.5e-6 then); the kernel at the clamp with a full-size draw stays held against the fp32 expression in test_gpu_training.py."""
import collections

import torch
import torch.nn.functional as F

from case_util import relerr_zero_exact as relerr, seq_mask as _seq_mask  # noqa: F401

GRAD_ABS = 2e-6
GRAD_REL = 1e-4                 # the project's per-op gradient bound
FWD_REL = 1e-5                  # the project's bound for fp32 forward ops
EPS = 1e-5
CS_REL = 1e-5                   # |dg - ref| <= CS_REL |dy| |f|
FORWARD = ("out", "ctx", "stat_max", "stat_inv", "mean", "rstd", "y", "df", "xt", "zm", "loss")


def cap(name):
    return FWD_REL if name in FORWARD else GRAD_REL


def bound(e32, name):
    return min(4.0 * e32 + GRAD_ABS, cap(name))


def ratioerr(got, ref):
    """max |got / ref - 1|, element-wise."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float(((got - ref) / ref).abs().max())


def _lens(B, W):
    """Ragged columns: one full utterance, then one of length 1, then one cut mid-row; repeated."""
    return [(W, 1, max(1, W // 2 + 1))[b % 3] for b in range(B)]


KINDS = ("plain", "offset30", "offset40", "offset300", "short", "saturated")
OFFSET_STD = {"offset30": 1.0, "offset40": 0.75, "offset300": 0.1}          # y = 30 + std * randn


def _norm_data(kind, g, B, C, H, W, mask):
    r = torch.randn(B, C, H, W, generator=g)
    if kind in OFFSET_STD:
        return 30.0 + OFFSET_STD[kind] * r
    if kind == "short":
        bias = 1.0 + 0.3 * torch.randn(C, generator=g)
        return bias[None, :, None, None] + r * mask[:, None, None, :]
    return 2.0 * r + 0.3


def errors(fam, got, ref):
    """{tensor: e} of `got` (a dict of the family's held tensors: the fp32 reference, a restatement, or what the kernels returned)
    against the float64 reference `ref`, each in its own norm (module docstring).  `ref` carries the scales."""
    e = {}
    for n in HELD[fam]:
        if n not in ref or ref[n] is None:
            continue
        if n == "mean":
            e[n] = relerr(got[n], ref[n], ref["y_max"])
        elif n in ("rstd", "stat_inv"):
            e[n] = ratioerr(got[n], ref[n])
        elif n == "dk":
            e[n] = relerr(got[n], ref[n], ref["dk_scale"])
        elif n == "dg_cs":
            e[n] = relerr(got[n], ref[n], ref["cs_scale"])
        else:
            e[n] = relerr(got[n], ref[n])
    return e


def passes(name, e, e32):
    """The GPU bound of one tensor."""
    if name == "stat_max":
        return e == 0.0
    if name == "dg_cs":
        return e <= CS_REL
    return e <= bound(e32, name)


HELD = {"GN": ("out", "mean", "rstd", "dy", "dgamma", "dbeta", "dtb"), "IN": ("out", "mean", "rstd", "dy", "dgamma", "dbeta"),
        "AT": ("out", "ctx", "stat_max", "stat_inv", "dq", "dk", "dv"), "RZ": ("y", "df", "dg", "dg_cs"), "NZ": ("xt", "zm", "loss", "geps")}

# what is held of a narrowed kind (module docstring); every other kind holds all of HELD
HELD_ONLY = {("GN", "offset300"): ("mean", "rstd", "dtb"), ("IN", "offset300"): ("mean", "rstd", "dy", "dgamma", "dbeta")}


def is_held(fam, kind, name):
    return name in HELD_ONLY.get((fam, kind), HELD[fam])


# caps on e_ref32 per family and data kind: {tensor: cap}, "*" for every held tensor not named -- about twice the maxima measured on
# the CPU; 4 x cap stays under the tensor's hard cap, so no case can fail on its reference alone
_NORM_CAP = {"plain": {"*": 1.2e-6, "dy": 5e-6}, "short": {"*": 1.2e-6}, "saturated": {"*": 1.2e-6}, "offset30": {"*": 2.5e-6, "dy": 4e-6, "dgamma": 1.6e-5},
             "offset40": {"*": 2.5e-6, "dy": 6e-6, "dgamma": 2.5e-5}, "offset300": {"*": 4e-7, "dy": 1.25e-5, "dgamma": 1.25e-5, "dbeta": 1.25e-5}}
E32_CAP = {"GN": _NORM_CAP, "IN": _NORM_CAP, "AT": {k: {"*": 1.3e-6} for k in ("flat", "peaked", "shifted", "late-max", "early-max")},
           "RZ": {"random": {"*": 8e-7}, "aligned": {"*": 8e-7}}, "NZ": {"t": {"*": 2.5e-6, "geps": 3.5e-6}}}


def e32_cap(fam, kind, name):
    d = E32_CAP[fam][kind]
    return d.get(name, d["*"])


# ============================================================================================================== GN: GroupNorm + Mish
GnCase = collections.namedtuple("GnCase", "id B C H W groups kind tb")
_GN_CROSSED = ((2, 16, 5, 7, 8), (2, 8, 4, 9, 8), (3, 64, 8, 131, 8))
_GN_PLAIN = ((1, 32, 32, 32, 4), (1, 512, 1, 16, 8), (40, 8, 1, 4, 8))
GN_CASES = ([GnCase("gn-b%d-c%d-%dx%d-g%d-%s-tb" % (s + (k,)), *s, k, True) for s in _GN_CROSSED for k in KINDS] +
            [GnCase("gn-b%d-c%d-%dx%d-g%d-plain-tb" % s, *s, "plain", True) for s in _GN_PLAIN] +
            [GnCase("gn-b%d-c%d-%dx%d-g%d-plain" % s, *s, "plain", False) for s in _GN_CROSSED])
GN_BY_ID = {c.id: c for c in GN_CASES}


def gn_inputs(c):
    g = torch.Generator().manual_seed(4000 + GN_CASES.index(c))
    mask = _seq_mask(_lens(c.B, c.W), c.W)
    y = _norm_data(c.kind, g, c.B, c.C, c.H, c.W, mask)
    gamma = 1.0 + 0.1 * torch.randn(c.C, generator=g)
    if c.kind == "saturated":
        gamma = gamma * 15.0
    return dict(y=y, gamma=gamma, beta=0.1 * torch.randn(c.C, generator=g), mask=mask, tb=torch.randn(c.B, c.C, generator=g) if c.tb else None,
                dout=torch.randn(c.B, c.C, c.H, c.W, generator=g))


def _region_stats(y, B, regions, unbiased=False):
    r = y.reshape(B, regions, -1)
    mean = r.mean(-1)
    return mean, 1.0 / torch.sqrt(r.var(-1, unbiased=unbiased) + EPS)


def gn_reference(c, d, dtype=torch.float64):
    """Mish(GroupNorm(y)) * mask + tb and its gradients by autograd; (mean, rstd) per (sample, group) from the plain expressions."""
    y, gamma, beta = (d[n].clone().to(dtype).requires_grad_(True) for n in ("y", "gamma", "beta"))
    tb = d["tb"].clone().to(dtype).requires_grad_(True) if c.tb else None
    out = F.mish(F.group_norm(y, c.groups, gamma, beta, EPS)) * d["mask"].to(dtype)[:, None, None, :]
    if c.tb:
        out = out + tb[:, :, None, None]
    out.backward(d["dout"].to(dtype))
    mean, rstd = _region_stats(y.detach(), c.B, c.groups)
    return dict(out=out.detach(), mean=mean, rstd=rstd, dy=y.grad, dgamma=gamma.grad, dbeta=beta.grad, dtb=tb.grad if c.tb else None,
                y_max=float(d["y"].abs().max()))


def mish_and_grad(z):
    """(Mish(z), Mish'(z)) = (z t, t + z sigmoid(z) (1 - t^2)) with t = tanh(softplus(z))  (csrc/train_norm.hip)."""
    t = torch.tanh(F.softplus(z, threshold=1e9))
    return z * t, t + z * torch.sigmoid(z) * (1.0 - t * t)


def gn_manual(c, d, mistake=None):
    """x_hat = (y - mean) rstd per (sample, group), z = x_hat gamma + beta, out = Mish(z) mask + tb;  dz = dout mask Mish'(z),
    dbeta = sum dz, dgamma = sum dz x_hat, dtb = sum_hw dout, dy = rstd (dz gamma - c1 - x_hat c2) with (c1, c2) the region means of
    (gamma dz, gamma dz x_hat)."""
    B, C, G = c.B, c.C, c.groups
    y, gamma, beta, dout = (d[n].double() for n in ("y", "gamma", "beta", "dout"))
    m = d["mask"].double()[:, None, None, :]
    src = y * m if mistake == "stats_over_masked_input" else y
    mean, rstd = _region_stats(src, B, G, unbiased=mistake == "unbiased_variance")
    shape = (B, G, C // G, c.H, c.W)
    mu, rs = mean.view(B, G, 1, 1, 1), rstd.view(B, G, 1, 1, 1)
    xh = ((y.view(shape) - mu) * rs).view(B, C, c.H, c.W)
    ga, be = gamma.view(1, C, 1, 1), beta.view(1, C, 1, 1)
    mi, dmi = mish_and_grad(xh * ga + be)
    res = dict(mean=mean, rstd=rstd, dtb=None)
    if c.tb:
        tb = d["tb"].double()[:, :, None, None]
        res["out"] = (mi + tb) * m if mistake == "tb_before_mask" else mi * m + tb
        res["dtb"] = (dout * m if mistake == "tb_before_mask" else dout).sum((2, 3))
    else:
        res["out"] = mi * m
    dz = dout * m * dmi
    res["dbeta"] = dz.sum((0, 2, 3))
    res["dgamma"] = ((dout * dmi if mistake == "dgamma_without_mask" else dz) * xh).sum((0, 2, 3))
    c1 = (dz * ga).view(shape).mean((2, 3, 4), keepdim=True)
    c2 = (dz * ga * xh).view(shape).mean((2, 3, 4), keepdim=True)
    if mistake == "dy_without_xhat_c2":
        c2 = torch.zeros_like(c2)
    res["dy"] = (rs * ((dz * ga).view(shape) - c1 - xh.view(shape) * c2)).view(B, C, c.H, c.W)
    return res


GN_MISTAKES = ("unbiased_variance", "stats_over_masked_input", "tb_before_mask", "dy_without_xhat_c2", "dgamma_without_mask")

# =========================================================================================================== IN: InstanceNorm2d + GLU
InCase = collections.namedtuple("InCase", "id B C H W kind")
IN_CASES = [InCase("in-b%d-c%d-%dx%d-%s" % (s + (k,)), *s, k) for s in ((2, 4, 5, 7), (1, 3, 16, 16), (2, 8, 8, 131)) for k in KINDS]
IN_BY_ID = {c.id: c for c in IN_CASES}


def in_inputs(c):
    """y [B, 2C, H, W]: the value half, then the gate half."""
    g = torch.Generator().manual_seed(5000 + IN_CASES.index(c))
    y = _norm_data(c.kind, g, c.B, 2 * c.C, c.H, c.W, _seq_mask(_lens(c.B, c.W), c.W))
    gamma = 1.0 + 0.1 * torch.randn(2 * c.C, generator=g)
    if c.kind == "saturated":
        gamma[c.C:] *= 15.0
    return dict(y=y, gamma=gamma, beta=0.1 * torch.randn(2 * c.C, generator=g), dout=torch.randn(c.B, c.C, c.H, c.W, generator=g))


def _in_stats(mean, rstd, B, C):
    """[B][C][4] = mean_a, rstd_a, mean_g, rstd_g -> (means [B, C, 2], rstds [B, C, 2])."""
    return torch.stack((mean[:, :C], mean[:, C:]), -1), torch.stack((rstd[:, :C], rstd[:, C:]), -1)


def in_reference(c, d, dtype=torch.float64):
    y, gamma, beta = (d[n].clone().to(dtype).requires_grad_(True) for n in ("y", "gamma", "beta"))
    out = F.glu(F.instance_norm(y, weight=gamma, bias=beta, use_input_stats=True, eps=EPS), dim=1)
    out.backward(d["dout"].to(dtype))
    mean, rstd = _in_stats(*_region_stats(y.detach(), c.B, 2 * c.C), c.B, c.C)
    return dict(out=out.detach(), mean=mean, rstd=rstd, dy=y.grad, dgamma=gamma.grad, dbeta=beta.grad, y_max=float(d["y"].abs().max()))


def in_manual(c, d, mistake=None):
    """a = x_hat_a gamma_a + beta_a, s = sigmoid(x_hat_g gamma_g + beta_g), out = a s;  da = dout s, dg = dout a s (1 - s); per plane
    dgamma = sum d x_hat, dbeta = sum d, dy = gamma rstd (d - mean(d) - x_hat mean(d x_hat))."""
    B, C = c.B, c.C
    y, gamma, beta, dout = (d[n].double() for n in ("y", "gamma", "beta", "dout"))
    mean, rstd = _region_stats(y, B, 2 * C)
    if mistake == "shared_statistic":            # one (mean, rstd) over both planes of a channel pair
        pm, pr = _region_stats(torch.cat((y[:, :C], y[:, C:]), 2), B, C)
        mean, rstd = torch.cat((pm, pm), 1), torch.cat((pr, pr), 1)
    xh = (y - mean[:, :, None, None]) * rstd[:, :, None, None]
    v = xh * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    a, s = v[:, :C], torch.sigmoid(v[:, C:])
    da = dout * s
    dg = dout * a * s if mistake == "gate_grad_without_one_minus_sigma" else dout * a * s * (1.0 - s)
    dv = torch.cat((da, dg), 1)
    m1, m2 = dv.mean((2, 3), keepdim=True), (dv * xh).mean((2, 3), keepdim=True)
    dy = gamma.view(1, -1, 1, 1) * rstd[:, :, None, None] * (dv - m1 - xh * m2)
    ms, rs = _in_stats(mean, rstd, B, C)
    return dict(out=a * s, mean=ms, rstd=rs, dy=dy, dgamma=(dv * xh).sum((0, 2, 3)), dbeta=dv.sum((0, 2, 3)))


IN_MISTAKES = ("shared_statistic", "gate_grad_without_one_minus_sigma")

# =========================================================================================================== AT: LinearAttention core
AtCase = collections.namedtuple("AtCase", "id N regime")
AT_B, AT_HEADS, AT_D, AT_SLICE = 2, 4, 32, 512
AT_NS = (1, 7, 64, 65, 257, 512, 513, 1025)
AT_CASES = ([AtCase("attn-n%d-%s" % (n, r), n, r) for n in AT_NS for r in ("flat", "peaked", "shifted")] +
            [AtCase("attn-n%d-%s" % (n, r), n, r) for n in AT_NS if n > AT_SLICE for r in ("late-max", "early-max")])
AT_BY_ID = {c.id: c for c in AT_CASES}


def at_inputs(c):
    """qkv [2, 384, 1, N] = q | k | v, each 4 heads x 32; dout [2, 128, 1, N]."""
    g = torch.Generator().manual_seed(6000 + AT_CASES.index(c))
    C, N = AT_HEADS * AT_D, c.N
    q, k, v = (torch.randn(AT_B, C, 1, N, generator=g) for _ in range(3))
    k = k * (12.0 if c.regime == "peaked" else 0.9)
    if c.regime == "shifted":
        k[:, 1::2] += 80.0                               # without the max subtraction exp overflows
    last = AT_SLICE * ((N - 1) // AT_SLICE)              # first pixel of the last slice
    if c.regime == "late-max":
        k[..., :last] -= 100.0                           # every earlier slice's weight e^{m_s - M} underflows
    if c.regime == "early-max":
        k[..., AT_SLICE:] -= 100.0
    return dict(qkv=torch.cat((q, k, v), 1).contiguous(), dout=torch.randn(AT_B, C, 1, N, generator=g))


def _heads(x):
    return x.reshape(AT_B, AT_HEADS, AT_D, -1)


def _split(qkv):
    C = AT_HEADS * AT_D
    return _heads(qkv[:, :C]), _heads(qkv[:, C:2 * C]), _heads(qkv[:, 2 * C:])


def at_reference(c, d, dtype=torch.float64):
    """diffusion.py:90-100 between to_qkv and to_out, and its gradient by autograd."""
    qkv = d["qkv"].clone().to(dtype).requires_grad_(True)
    q, k, v = _split(qkv)
    ks = k.softmax(dim=-1)
    ctx = torch.einsum("bhdn,bhen->bhde", ks, v)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(AT_B, AT_HEADS * AT_D, 1, c.N)
    out.backward(d["dout"].to(dtype))
    C = AT_HEADS * AT_D
    dq, dk, dv = qkv.grad[:, :C], qkv.grad[:, C:2 * C], qkv.grad[:, 2 * C:]
    kd = k.detach()
    M = kd.max(-1).values
    res = dict(out=out.detach(), ctx=ctx.detach(), stat_max=M, stat_inv=1.0 / torch.exp(kd - M.unsqueeze(-1)).sum(-1), dq=dq, dk=dk, dv=dv)
    if dtype == torch.float64:        # the scale of dk's two cancelling terms: k~ t, t[d,n] = sum_e dctx[d][e] v[e,n]
        dctx = torch.einsum("bhdn,bhen->bhde", q.detach(), _heads(d["dout"].double()))
        kt = ks.detach() * torch.einsum("bhde,bhen->bhdn", dctx, v.detach())
        res["dk_scale"] = max(float(dk.abs().max()), float(kt.abs().max()))
    return res


def at_manual(c, d, mistake=None):
    """The header of csrc/train_attn.hip in float64.  Forward in the kernels' sliced form: per slice of 512 pixels the row maximum m_s,
    S_s = sum e^{k - m_s} and rec_s[d][e] = sum e^{k - m_s} v[e]; combined with the weights e^{m_s - M}.  Backward: dq = ctx dout,
    dctx = q dout^T, dv = k~^T dctx, dk = k~ (dctx v - r), r_d = sum_e dctx[d][e] ctx[d][e]."""
    q, k, v = _split(d["qkv"].double())
    do = _heads(d["dout"].double())
    if mistake == "softmax_over_channels":
        ks = k.softmax(dim=-2)
        ctx = torch.einsum("bhdn,bhen->bhde", ks, v)
        M = k.max(-1).values
        inv = 1.0 / torch.exp(k - M.unsqueeze(-1)).sum(-1)
    else:
        ms, Ss, recs = [], [], []
        for n0 in range(0, c.N, AT_SLICE):
            ksl, vsl = k[..., n0:n0 + AT_SLICE], v[..., n0:n0 + AT_SLICE]
            m = ksl.max(-1).values
            p = torch.exp(ksl - m.unsqueeze(-1))
            ms.append(m), Ss.append(p.sum(-1)), recs.append(torch.einsum("bhdn,bhen->bhde", p, vsl))
        M = torch.stack(ms).max(0).values
        w = [torch.ones_like(M) if mistake == "combine_ignores_slice_weights" else torch.exp(m - M) for m in ms]
        S = sum(s * wi for s, wi in zip(Ss, w))
        ctx = sum(r * wi.unsqueeze(-1) for r, wi in zip(recs, w)) / S.unsqueeze(-1)
        inv = 1.0 / S
        ks = torch.exp(k - M.unsqueeze(-1)) * inv.unsqueeze(-1)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q)
    dq = torch.einsum("bhed,bhen->bhdn" if mistake == "ctx_transposed_in_dq" else "bhde,bhen->bhdn", ctx, do)
    dctx = torch.einsum("bhdn,bhen->bhde", q, do)
    r = torch.zeros_like(M) if mistake == "dk_without_r" else (dctx * ctx).sum(-1)
    dk = ks * (torch.einsum("bhde,bhen->bhdn", dctx, v) - r.unsqueeze(-1))
    dv = torch.einsum("bhdn,bhde->bhen", ks, dctx)
    sh = (AT_B, AT_HEADS * AT_D, 1, c.N)
    return dict(out=out.reshape(sh), ctx=ctx, stat_max=M, stat_inv=inv, dq=dq.reshape(sh), dk=dk.reshape(sh), dv=dv.reshape(sh))


AT_MISTAKES = ("softmax_over_channels", "dk_without_r", "ctx_transposed_in_dq", "combine_ignores_slice_weights")

# ========================================================================================================================== RZ: Rezero
RzCase = collections.namedtuple("RzCase", "id n dy_kind")
RZ_FULL_GRID = 2048 * 256 * 4        # floats of one pass of the full grid of float4 loads
RZ_CASES = [RzCase("rezero-n%d-%s" % (n, k), n, k) for n in (4, 1020, 1028, RZ_FULL_GRID + 4) for k in ("random", "aligned")]
RZ_BY_ID = {c.id: c for c in RZ_CASES}
RZ_G = 0.3


def rz_inputs(c):
    g = torch.Generator().manual_seed(7000 + RZ_CASES.index(c))
    f, x = torch.randn(c.n, generator=g), torch.randn(c.n, generator=g)
    dy = torch.randn(c.n, generator=g) if c.dy_kind == "random" else f.abs()
    return dict(f=f, x=x, g=torch.tensor([RZ_G]), dy=dy)


def rz_reference(c, d, dtype=torch.float64):
    f, g = (d[n].clone().to(dtype).requires_grad_(True) for n in ("f", "g"))
    y = f * g + d["x"].to(dtype)
    y.backward(d["dy"].to(dtype))
    res = dict(y=y.detach(), df=f.grad, cs_scale=float(d["dy"].double().norm() * d["f"].double().norm()))
    res["dg_cs" if c.dy_kind == "random" else "dg"] = g.grad
    return res


def rz_manual(c, d, mistake=None):
    f, x, dy, g = (d[n].double() for n in ("f", "x", "dy", "g"))
    res = dict(y=f * g + x, df=dy * g)
    res["dg_cs" if c.dy_kind == "random" else "dg"] = (dy * (x if mistake == "dg_from_x" else f)).sum().view(1)
    return res


RZ_MISTAKES = ("dg_from_x",)

# ==================================================================================================== NZ: noising and score-loss head
NzCase = collections.namedtuple("NzCase", "id B F T t")
NZ_CASES = [NzCase("noise-b3-f80-t52", 3, 80, 52, (1.0, 0.4, 1e-5)), NzCase("noise-b2-f5-t51", 2, 5, 51, (1e-5, 1.0))]
NZ_BY_ID = {c.id: c for c in NZ_CASES}
BETA_MIN, BETA_MAX = 0.05, 20.0
NZ_SMALL_T, NZ_SMALL_Z = 1e-3, 0.1           # the narrowed kind (module docstring)


def nz_inputs(c):
    g = torch.Generator().manual_seed(8000 + c.T)
    x0, mu, z, eps = (torch.randn(c.B, c.F, c.T, generator=g) for _ in range(4))
    t = torch.tensor(c.t, dtype=torch.float32)
    z = z * torch.where(t < NZ_SMALL_T, NZ_SMALL_Z, 1.0)[:, None, None]
    mask = _seq_mask([(c.T, max(1, c.T // 2 + 1), 1)[b % 3] for b in range(c.B)], c.T)
    return dict(x0=x0, mu=mu, z=z, eps=eps, t=t, mask=mask, inv_denom=1.0 / (float(mask.sum()) * c.F))


def nz_reference(c, d, dtype=torch.float64):
    """forward_diffusion given the draw z (diffusion.py:244-252) and loss_t's reduction (:285-287), d loss / d eps by autograd."""
    x0, mu, z, t = (d[n].to(dtype) for n in ("x0", "mu", "z", "t"))
    mask = d["mask"].to(dtype)[:, None]
    tt = t[:, None, None]
    cum = BETA_MIN * tt + 0.5 * (BETA_MAX - BETA_MIN) * tt ** 2
    mean = x0 * torch.exp(-0.5 * cum) + mu * (1.0 - torch.exp(-0.5 * cum))
    xt = (mean + z * torch.sqrt(1.0 - torch.exp(-cum))) * mask
    zm = z * mask
    eps = d["eps"].clone().to(dtype).requires_grad_(True)
    loss = torch.sum((eps * torch.sqrt(1.0 - torch.exp(-cum)) + zm) ** 2) * d["inv_denom"]
    loss.backward()
    return dict(xt=xt, zm=zm, loss=loss.detach(), geps=eps.grad)


FAMILIES = {"GN": (GN_CASES, gn_inputs, gn_reference, gn_manual, GN_MISTAKES), "IN": (IN_CASES, in_inputs, in_reference, in_manual, IN_MISTAKES),
            "AT": (AT_CASES, at_inputs, at_reference, at_manual, AT_MISTAKES), "RZ": (RZ_CASES, rz_inputs, rz_reference, rz_manual, RZ_MISTAKES),
            "NZ": (NZ_CASES, nz_inputs, nz_reference, None, ())}


def kind_of(fam, c):
    return {"GN": lambda: c.kind, "IN": lambda: c.kind, "AT": lambda: c.regime, "RZ": lambda: c.dy_kind, "NZ": lambda: "t"}[fam]()
