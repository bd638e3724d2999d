"""Catalogue of single-op TRAINING cases of the encoders' two fp32 VALU ops (csrc/enc_train.hip): the backward of the windowed
relative-position attention core (with the training forward and its dropout multiplier) and the backward of LayerNorm with its five
flags.  Cases and input builders are those of tests/enc_op_cases.py, unchanged; this module adds the upstream gradients, the float64
references and the bounds.

  upstream   dout = torch.randn(B, C, L, generator = manual_seed(77)) for attention, seed 78 for LayerNorm
  reference  float64 autograd through oracle.encoder_oracle.attention_core / layer_norm; e_ref32 = the same autograd in fp32 torch on
             the CPU.  Dropout cases (a fixed Bernoulli(0.9) / 0.9 multiplier on the probabilities): autograd through att_direct_train,
             a float64 restatement with the direct index r = j - i + w that the CPU test holds to attention_core at 1e-12 without dropout
  error      per gradient tensor  e = max |got - ref64| / max |ref64|  (a reference that is exactly zero -- the score gradients of a
             one-key softmax -- asks for exact zeros: e = 0 then, inf otherwise)
  GPU bound  e <= 4 e_ref32 + 2e-6 and e <= 1e-4 (the project's gradient bound); in the saturated regime dq, dk and dek are only held
             to be finite: fp32 autograd itself is 100 % off there (the gradients vanish)
  caps on e_ref32, asserted by tests/test_enc_train_op_cases_cpu.py: attention init 2e-6, peaked 2.5e-5, saturated dv / dev 2e-6;
             LayerNorm 2e-6, dgamma of the `offset` data kind 4e-6

att_backward_manual / ln_backward_manual state the backward formulas the kernels implement, in float64, and restate backward mistakes
on them (ATT_TRAIN_MISTAKES, LN_TRAIN_MISTAKES); the CPU test shows the formulas equal autograd and the bound rejects each mistake."""
import collections
import math

import torch

import enc_op_cases as K
from case_util import relerr_zero_exact as relerr, seq_mask  # noqa: F401
from oracle import encoder_oracle as E

GRAD_ABS = 2e-6
GRAD_REL = 1e-4                 # the project's gradient bound
E32_CAP = {"init": 2e-6, "peaked": 2.5e-5, "saturated": 2e-6}
LN_E32_CAP, LN_E32_CAP_OFFSET_DGAMMA = 2e-6, 4e-6
ATT_GRADS = ("dq", "dk", "dv", "dek", "dev")
LN_GRADS = ("da", "dbres", "dgamma", "dbeta")
SATURATED_FINITE_ONLY = ("dq", "dk", "dek")


def bound(e32):
    return min(4.0 * e32 + GRAD_ABS, GRAD_REL)


def held(c, name):
    """Whether gradient `name` of attention case c is held to the bound (else: finite only)."""
    return not (c.regime == "saturated" and name in SATURATED_FINITE_ONLY)


# =============================================================================================================== attention
LONG = K.AttCase("att-train-h1-dk96-L1025-w4-init", 1, 1, 96, 1025, 4, "init", (1000,), ())      # many key blocks, 17 key tiles
ATT_TRAIN_CASES = list(K.ATT_SMALL) + [LONG]
ATT_TRAIN_BY_ID = {c.id: c for c in ATT_TRAIN_CASES}
# the dropout cases: every regime, padding and a fully masked item, no window / the widest one, a narrow head
DROP_IDS = ("att-len-h2-dk48-L65-w4-init", "att-len-h2-dk48-L17-w4-peaked", "att-len-h2-dk48-L130-w4-saturated",
            "att-win-h2-dk48-L17-w0-init", "att-win-h2-dk48-L17-w8-peaked", "att-width-h8-dk10-L65-w4-init")
DROP_P = 0.1


def att_train_inputs(c):
    """K.att_inputs for the cases of enc_op_cases; the long case is built the same way (init regime) from seeds of its own."""
    if c.id in K.ATT_BY_ID:
        return K.att_inputs(c)
    assert c is LONG
    g = torch.Generator().manual_seed(5999)
    B, H, dk, L, w = c.B, c.heads, c.dk, c.L, c.window
    C = H * dk
    mask = seq_mask(c.lens, L)
    sd = E.make_state("mel", n_feats=4, C=C, filt=C, n_heads=H, n_layers=1, window=w, seed=399)
    p = "encoder.attn_layers.0."
    x = torch.randn(B, C, L, generator=g) * mask.unsqueeze(1)
    q, k, v = (E.conv(sd, p + n, x, 1) for n in ("conv_q.", "conv_k.", "conv_v."))
    pad = (mask == 0).unsqueeze(1)
    sq, sk, sv = float(q.std()), float(k.std()), float(v.std())
    q = torch.where(pad, 100.0 * sq * torch.randn(B, C, L, generator=g), q)
    k = torch.where(pad, 100.0 * sk * torch.randn(B, C, L, generator=g), k)
    alt = (1.0 - 2.0 * (torch.arange(L) % 2)).view(1, 1, L) * (4.0 * sv * (1.0 + torch.rand(1, C, 1, generator=g)))
    v = torch.where(pad, alt.expand(B, C, L), v)
    return dict(q=q.contiguous(), k=k.contiguous(), v=v.contiguous(), mask=mask, ek=sd[p + "emb_rel_k"][0].contiguous(),
                ev=sd[p + "emb_rel_v"][0].contiguous())


def att_dout(c):
    return torch.randn(c.B, c.heads * c.dk, c.L, generator=torch.Generator().manual_seed(77))


def att_drop(c):
    """The fixed dropout multiplier of a dropout case: Bernoulli(1 - DROP_P) / (1 - DROP_P), [B, H, L, L] fp32."""
    keep = torch.rand(c.B, c.heads, c.L, c.L, generator=torch.Generator().manual_seed(79)) < (1.0 - DROP_P)
    return keep.float() / (1.0 - DROP_P)


def _band(c):
    """rc [L, L] = clamp(j - i + w), inside [L, L] = |j - i| <= w  (None, None without a window)."""
    if not c.window:
        return None, None
    L, w = c.L, c.window
    ii, jj = torch.meshgrid(torch.arange(L), torch.arange(L), indexing="ij")
    r = jj - ii + w
    return r.clamp(0, 2 * w), (r >= 0) & (r <= 2 * w)


def att_direct_train(c, q, k, v, mask, ek, ev, drop=None):
    """The attention core with the direct index r = j - i + w and the dropout multiplier on the probabilities, differentiable, in the
    dtype of its arguments (q, k, v [B, C, L]; ek, ev [2w+1, dk] or None; drop [B, H, L, L] or None) -> [B, C, L]."""
    B, H, dk, L = c.B, c.heads, c.dk, c.L
    f = lambda x: x.view(B, H, dk, L).transpose(2, 3)
    qh, kh, vh = f(q), f(k), f(v)
    inv = 1.0 / math.sqrt(dk)
    scores = qh @ kh.transpose(-2, -1) * inv
    rc, inside = _band(c)
    if c.window:
        rel = torch.einsum("bhid,rd->bhir", qh, ek).gather(-1, rc.view(1, 1, L, L).expand(B, H, L, L)) * inside.to(q.dtype)
        scores = scores + rel * inv
    m = mask.to(q.dtype)
    scores = scores.masked_fill(m.view(B, 1, L, 1) * m.view(B, 1, 1, L) == 0, -1e4)
    p = torch.softmax(scores, -1)
    pd = p if drop is None else p * drop.to(q.dtype)
    out = pd @ vh
    if c.window:
        out = out + torch.einsum("bhij,ijd->bhid", pd, ev[rc] * inside.unsqueeze(-1).to(q.dtype))
    return out.transpose(2, 3).contiguous().view(B, H * dk, L)


def att_grads(c, d, dtype=torch.float64, drop=None, direct=False):
    """dict(out, dq, dk, dv, dek, dev) by autograd in `dtype` (dek = dev = None without a window): through attention_core, or through
    att_direct_train when a dropout multiplier is given (or direct=True)."""
    leaf = {n: (None if d[n] is None else d[n].to(dtype).clone().requires_grad_(True)) for n in ("q", "k", "v", "ek", "ev")}
    if drop is not None or direct:
        out = att_direct_train(c, leaf["q"], leaf["k"], leaf["v"], d["mask"], leaf["ek"], leaf["ev"], drop)
    else:
        out = K.att_reference(c, dict(d, **leaf), dtype)
    out.backward(att_dout(c).to(dtype))
    g = lambda n: None if leaf[n] is None else leaf[n].grad
    return dict(out=out.detach(), dq=g("q"), dk=g("k"), dv=g("v"), dek=g("ek"), dev=g("ev"))


ATT_TRAIN_MISTAKES = ("ds-kept-at-masked", "no-delta", "dek-no-inv", "r+1", "r-1", "drop-once")


def att_backward_manual(c, d, drop=None, mistake=None):
    """The backward formulas of csrc/enc_train.hip in float64 (the header of that file), and backward mistakes restated on them:
      ds-kept-at-masked  ds not zeroed where the score was replaced by -1e4        no-delta   the - sum_j p dp term dropped
      dek-no-inv         dEk without the 1 / sqrt(dk)                              r+1, r-1   the band index off by one in the backward
      drop-once          dp = dpd: the multiplier applied to pd (forward) but not again to the gradient (None without dropout)
    -> dict(dq, dk, dv, dek, dev)."""
    assert mistake is None or mistake in ATT_TRAIN_MISTAKES
    if mistake == "drop-once" and drop is None:
        return None
    if mistake in ("dek-no-inv", "r+1", "r-1") and not c.window:
        return None
    B, H, dk, L, w = c.B, c.heads, c.dk, c.L, c.window
    f = lambda x: x.double().view(B, H, dk, L).transpose(2, 3)
    q, k, v, do = f(d["q"]), f(d["k"]), f(d["v"]), f(att_dout(c))
    inv = 1.0 / math.sqrt(dk)
    s = q @ k.transpose(-2, -1) * inv
    rc, inside = _band(c)
    if w:
        ek, ev = d["ek"].double(), d["ev"].double()
        s = s + torch.einsum("bhid,rd->bhir", q, ek).gather(-1, rc.view(1, 1, L, L).expand(B, H, L, L)) * inside * inv
    m = d["mask"].double()
    dead = (m.view(B, 1, L, 1) * m.view(B, 1, 1, L) == 0).expand(B, H, L, L)
    p = torch.softmax(s.masked_fill(dead, -1e4), -1)
    dm = torch.ones_like(p) if drop is None else drop.double()
    pd = p * dm
    if w:
        shift = {"r+1": 1, "r-1": -1}.get(mistake, 0)
        rb = rc + shift
        onehot = ((rb.unsqueeze(-1) == torch.arange(2 * w + 1).view(1, 1, -1)) & inside.unsqueeze(-1)).double()      # [L, L, 2w+1]
    dpd = do @ v.transpose(-2, -1)
    if w:
        dpd = dpd + torch.einsum("bhid,rd,ijr->bhij", do, ev, onehot)
    dv = pd.transpose(-2, -1) @ do
    dp = dpd if mistake == "drop-once" else dpd * dm
    delta = (p * dp).sum(-1, keepdim=True)
    ds = p * dp if mistake == "no-delta" else p * (dp - delta)
    if mistake != "ds-kept-at-masked":
        ds = ds.masked_fill(dead, 0.0)
    dq = ds @ k
    dkk = ds.transpose(-2, -1) @ q * inv
    dek = dev = None
    if w:
        dq = dq + torch.einsum("bhij,ijr,rd->bhid", ds, onehot, ek)
        dek = torch.einsum("bhij,ijr,bhid->rd", ds, onehot, q) * (1.0 if mistake == "dek-no-inv" else inv)
        dev = torch.einsum("bhij,ijr,bhid->rd", pd, onehot, do)
    dq = dq * inv
    back = lambda x: x.transpose(2, 3).contiguous().view(B, H * dk, L)
    return dict(dq=back(dq), dk=back(dkk), dv=back(dv), dek=dek, dev=dev)


# =============================================================================================================== LayerNorm
def ln_dout(c):
    return torch.randn(c.B, c.C, c.L, generator=torch.Generator().manual_seed(78))


def ln_grads(c, d, dtype=torch.float64):
    """dict(out, da, dbres, dgamma, dbeta) by autograd through oracle.encoder_oracle.layer_norm in `dtype` (dbres None without bres)."""
    leaf = {n: (None if d[n] is None else d[n].to(dtype).clone().requires_grad_(True)) for n in ("a", "bres", "gamma", "beta")}
    out = K.ln_reference(c, dict(d, **leaf), dtype)
    out.backward(ln_dout(c).to(dtype))
    g = lambda n: None if leaf[n] is None else leaf[n].grad
    return dict(out=out.detach(), da=g("a"), dbres=g("bres"), dgamma=g("gamma"), dbeta=g("beta"))


LN_TRAIN_MISTAKES = ("dgamma-no-out-mask", "relu-in-after-mask", "no-mean-terms")


def ln_backward_manual(c, d, mistake=None):
    """The backward formulas of enc_layernorm_bwd_kernel in float64, and mistakes restated on them (None where one cannot touch the case):
      dgamma-no-out-mask  dgamma / dbeta summed from dout instead of dout * out_mask
      relu-in-after-mask  ReLU' of relu_in evaluated on relu(a) * a_mask + bres, the wrong side of the mask and the residual
      no-mean-terms       dv = rstd * dxhat, the two mean terms dropped"""
    assert mistake is None or mistake in LN_TRAIN_MISTAKES
    if mistake == "dgamma-no-out-mask" and not (c.out_mask and min(c.lens) < c.L):
        return None
    if mistake == "relu-in-after-mask" and not (c.relu_in and c.bres):
        return None
    return _ln_manual(c, d, mistake)


def _ln_manual(c, d, mistake):
    t = lambda x: None if x is None else x.double()
    a, bres, gamma, beta = t(d["a"]), t(d["bres"]), t(d["gamma"]).view(1, -1, 1), t(d["beta"]).view(1, -1, 1)
    am = torch.ones(c.B, 1, c.L, dtype=torch.float64) if d["a_mask"] is None else t(d["a_mask"]).unsqueeze(1)
    om = torch.ones(c.B, 1, c.L, dtype=torch.float64) if d["out_mask"] is None else t(d["out_mask"]).unsqueeze(1)
    x = torch.relu(a) if c.relu_in else a
    x = x * am
    if bres is not None:
        x = x + bres
    mean = x.mean(1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(1, keepdim=True) + K.EPS)
    xh = (x - mean) * rstd
    dout = ln_dout(c).double()
    g = dout * om
    if c.relu_out:
        g = g * (xh * gamma + beta > 0)
    gp = dout * (xh * gamma + beta > 0) if (mistake == "dgamma-no-out-mask" and c.relu_out) else (dout if mistake == "dgamma-no-out-mask" else g)
    dgamma, dbeta = (gp * xh).sum((0, 2)), gp.sum((0, 2))
    dx = g * gamma
    dv = rstd * dx if mistake == "no-mean-terms" else rstd * (dx - dx.mean(1, keepdim=True) - xh * (dx * xh).mean(1, keepdim=True))
    da = dv * am
    if c.relu_in:
        if mistake == "relu-in-after-mask":
            da = da * (x > 0)
        else:
            da = da * (a > 0)
    return dict(da=da, dbres=dv if bres is not None else None, dgamma=dgamma, dbeta=dbeta)


Row = collections.namedtuple("Row", "name e e32 bound held")
