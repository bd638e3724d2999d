"""Catalogue of single-op cases of the encoder-decoder gradient path of GradTTS.compute_loss (csrc/glue_train.hip, gtts_conv_dgrad_small,
gtts_diffusion_noising_backward), with float64 references and float64 restatements of what the kernels compute.

  A  first-layer data gradient     dx of Conv2d_kxk(x * mask), cin 2 or 3, k 3 or 1           (model/_train_ops.py: MaskedConv3x3 / 1x1)
  B  noising backward              dx0, dmu of Diffusion.forward_diffusion                    (model/diffusion.py)
  C  alignment glue                model/tts.py:103-125 -- frames per token, duration loss, crop, mu_y = attn^T . mu_x, prior loss

  reference    float64 autograd of the repository's composition (`*_composition`: F.conv2d of the masked input; the module's own
               forward_diffusion; the lines of GradTTS.compute_loss between MAS and the decoder, with the window starts handed in instead
               of drawn); e_ref32 = the same autograd in fp32 torch on the CPU
  restatement  `*_manual`: the formulas of include/gradtts_abi.h in float64 (flipped-tap sum; d and 1 - d; index / gather / segment sum),
               with the mistakes of MISTAKES restated on them
  error        per tensor  e = max |got - ref64| / max |ref64|  (an all-zero reference asks for exact zeros)
  GPU bound    e <= 4 e_ref32 + 2e-6 and e <= 1e-4 (the project's per-op gradient bound, tests/enc_train_op_cases.py); copies and counts
               (idx, dur, first, y_c, mu_y) are compared with torch.equal
Paths are built from random monotone durations (every live token owns at least one frame, as MAS gives), never from MAS itself, so no
case hangs on a near-tie.  tests/test_glue_train_cases_cpu.py proves the restatements against the references and that the bound tells
every restated mistake from the contract."""
import collections
import importlib
import math
import types

import torch
import torch.nn.functional as F

from case_util import relerr_zero_exact as relerr, seq_mask as _seq_mask  # noqa: F401

GRAD_ABS = 2e-6
GRAD_REL = 1e-4
LOG_2PI = math.log(2 * math.pi)
G_DUR, G_PRIOR = 0.7, 1.3                 # upstream gradients of the two scalar losses in the C cases


def bound(e32):
    return min(4.0 * e32 + GRAD_ABS, GRAD_REL)


def _lens(B, W):
    """Ragged columns: one full sample, one cut mid-row, one of length 1."""
    return [W, max(1, W // 2 + 1), 1][:B]


# ======================================================================================================== A: first-layer data gradient
ACase = collections.namedtuple("ACase", "id B cin H W cout k")
A_CASES = [ACase("dgrad-b%d-c%d-%dx%d-o%d-k%d" % s, *s) for s in ((1, 2, 5, 4, 64, 3), (2, 3, 7, 68, 64, 1), (2, 2, 80, 44, 128, 3),
                                                                 (3, 3, 80, 172, 64, 3), (3, 2, 80, 172, 64, 1))]
A_BY_ID = {c.id: c for c in A_CASES}


def a_inputs(c):
    """dy with four times the energy on the first and last row and column (a flipped tap or a missing border shows there), weights
    of a fresh Conv2d's scale, ragged column mask [B, W]."""
    g = torch.Generator().manual_seed(1000 + c.W + c.cout + c.k)
    dy = torch.randn(c.B, c.cout, c.H, c.W, generator=g)
    for sl in ((..., 0, slice(None)), (..., -1, slice(None)), (..., slice(None), 0), (..., slice(None), -1)):
        dy[sl] *= 4.0
    w = torch.randn(c.cout, c.cin, c.k, c.k, generator=g) / math.sqrt(c.cin * c.k * c.k)
    return dict(dy=dy, w=w, mask=_seq_mask(_lens(c.B, c.W), c.W))


def a_composition(c, d, dtype=torch.float64):
    """dx by autograd through the module's forward: F.conv2d(x * mask, w, padding k // 2)."""
    x = torch.zeros(c.B, c.cin, c.H, c.W, dtype=dtype, requires_grad=True)
    y = F.conv2d(x * d["mask"].to(dtype)[:, None, None, :], d["w"].to(dtype), None, padding=c.k // 2)
    y.backward(d["dy"].to(dtype))
    return dict(dx=x.grad)


def a_manual(c, d, mistake=None):
    """dx[b,p,h,w] = mask[b,w] sum_co sum_taps dy[b,co,h-kh+r,w-kw+r] w[co,p,kh,kw] in float64, taps outside the plane zero."""
    dy, w, r = d["dy"].double(), d["w"].double(), c.k // 2
    dyp = F.pad(dy, (2 * r, 2 * r, 2 * r, 2 * r))
    dx = torch.zeros(c.B, c.cin, c.H, c.W, dtype=torch.float64)
    for kh in range(c.k):
        for kw in range(c.k):
            oh, ow = (kh - r, kw - r) if mistake == "taps_not_flipped" else (r - kh, r - kw)
            sl = dyp[:, :, 2 * r + oh:2 * r + oh + c.H, 2 * r + ow:2 * r + ow + c.W]
            dx += torch.einsum("bchw,cp->bphw", sl, w[:, :, kh, kw])
    if mistake != "column_mask_dropped":
        dx = dx * d["mask"].double()[:, None, None, :]
    return dict(dx=dx)


# ================================================================================================================ B: noising backward
BCase = collections.namedtuple("BCase", "id B F T t")
B_CASES = [BCase("noise-b1-f80-t4", 1, 80, 4, (0.5,)), BCase("noise-b3-f80-t44", 3, 80, 44, (1e-5, 0.5, 1.0 - 1e-5)),
           BCase("noise-b2-f5-t172", 2, 5, 172, (1.0 - 1e-5, 1e-5))]
B_BY_ID = {c.id: c for c in B_CASES}
B_MODES = ("dx0", "dmu", "both")
BETA_MIN, BETA_MAX = 0.05, 20.0


def b_inputs(c):
    g = torch.Generator().manual_seed(2000 + c.T)
    return dict(dxt=torch.randn(c.B, c.F, c.T, generator=g), x0=torch.randn(c.B, c.F, c.T, generator=g),
                mu=torch.randn(c.B, c.F, c.T, generator=g), mask=_seq_mask(_lens(c.B, c.T), c.T), t=torch.tensor(c.t, dtype=torch.float32))


def b_composition(c, d, dtype=torch.float64):
    """(dx0, dmu) by autograd through Diffusion.forward_diffusion's own torch branch (its noise draw does not enter the gradient)."""
    D = importlib.import_module("speech-backbones_amd.model.diffusion")
    x0 = d["x0"].clone().to(dtype).requires_grad_(True)
    mu = d["mu"].clone().to(dtype).requires_grad_(True)
    state = torch.get_rng_state()
    try:
        xt, _ = D.Diffusion.forward_diffusion(types.SimpleNamespace(beta_min=BETA_MIN, beta_max=BETA_MAX), x0, d["mask"].to(dtype)[:, None],
                                              mu, d["t"].to(dtype))
    finally:
        torch.set_rng_state(state)
    xt.backward(d["dxt"].to(dtype))
    return dict(dx0=x0.grad, dmu=mu.grad)


def b_manual(c, d, mistake=None):
    """dx0 = d mask dxt, dmu = (1 - d) mask dxt with d = exp(-cum / 2), cum = beta_min t + (beta_max - beta_min) t^2 / 2."""
    t = d["t"].double()[:, None, None]
    dec = torch.exp(-0.5 * (BETA_MIN * t + 0.5 * (BETA_MAX - BETA_MIN) * t * t))
    g = d["dxt"].double() * d["mask"].double()[:, None]
    a, b = (1.0 - dec, dec) if mistake == "decay_swapped" else (dec, 1.0 - dec)
    return dict(dx0=a * g, dmu=b * g)


# ================================================================================================================== C: alignment glue
CCase = collections.namedtuple("CCase", "id B F tx T out_size")
C_CASES = [CCase("glue-b%d-f%d-tx%d-T%d-%s" % (s[0], s[1], s[2], s[3], "full" if s[4] is None else "crop%d" % s[4]), *s)
           for s in ((3, 80, 7, 23, None), (3, 80, 7, 23, 8), (3, 80, 7, 23, 16), (2, 80, 40, 130, 48), (1, 5, 1, 3, None))]
C_BY_ID = {c.id: c for c in C_CASES}
C_COPIES = ("idx", "dur", "first", "y_c", "mu_y")
C_BOUNDED = ("dur_loss", "prior_loss", "dlogw", "dmu_x")


def c_inputs(c):
    """Padded tokens and frames (ragged x / y lengths), a random monotone path with at least one frame per live token, window starts
    that cut a token's run in two where the slack allows it, fixed upstream gradients."""
    g = torch.Generator().manual_seed(3000 + 7 * c.T + (c.out_size or 0))
    x_lens = [c.tx, max(1, c.tx * 2 // 3), max(1, c.tx // 3)][:c.B]
    y_lens = [c.T, max(x_lens[1], c.T * 11 // 20) if c.B > 1 else 0, max(x_lens[2], c.T // 3) if c.B > 2 else 0][:c.B]
    path = torch.zeros(c.B, c.tx, c.T)
    for b in range(c.B):
        cuts = (torch.randperm(y_lens[b] - 1, generator=g)[:x_lens[b] - 1] + 1).sort().values.tolist()
        edges = [0] + cuts + [y_lens[b]]
        for i in range(x_lens[b]):
            path[b, i, edges[i]:edges[i + 1]] = 1.0
    y = torch.randn(c.B, c.F, c.T, generator=g)
    pad = 1.0 - _seq_mask(y_lens, c.T)[:, None]
    # the uncropped composition hands y to the decoder as it is (padded frames are zeros in a data loader's batch); a crop multiplies
    # by its live mask, so there the padding may hold anything
    y = y * (1.0 - pad) if c.out_size is None else y * (1.0 - pad) + 50.0 * pad
    S = c.T if c.out_size is None else c.out_size
    starts = [0] * c.B
    if c.out_size is not None:
        tok = path.argmax(1)
        for b in range(c.B):
            slack = max(y_lens[b] - c.out_size, 0)
            inside = [s for s in range(1, slack + 1) if tok[b, s - 1] == tok[b, s]]
            starts[b] = inside[0] if inside else slack
    return dict(path=path, mu_x=torch.randn(c.B, c.F, c.tx, generator=g), logw=torch.randn(c.B, 1, c.tx, generator=g),
                x_mask=_seq_mask(x_lens, c.tx)[:, None], x_lengths=torch.tensor(x_lens), y=y, y_lengths=torch.tensor(y_lens),
                starts=starts, S=S, g_mu_y=torch.randn(c.B, c.F, S, generator=g))


def c_kept(c, d):
    return torch.clamp(d["y_lengths"], max=d["S"])


def c_composition(c, d, dtype=torch.float64):
    """model/tts.py:103-125, line for line, with the window starts handed in; gradients of G_DUR dur_loss + G_PRIOR prior_loss +
    sum(g_mu_y mu_y) w.r.t. logw and mu_x."""
    U = importlib.import_module("speech-backbones_amd.model.utils")
    attn, y, x_mask = d["path"].to(dtype), d["y"].to(dtype), d["x_mask"].to(dtype)
    x_lengths, y_lengths, out_size, frames = d["x_lengths"], d["y_lengths"], c.out_size, c.T
    mu_x = d["mu_x"].clone().to(dtype).requires_grad_(True)
    logw = d["logw"].clone().to(dtype).requires_grad_(True)
    y_mask = U.sequence_mask(y_lengths, frames).unsqueeze(1).to(x_mask)

    frames_per_token = attn.sum(-1).unsqueeze(1)
    dur_loss = U.duration_loss(logw, torch.log(1e-8 + frames_per_token) * x_mask, x_lengths)
    if out_size is not None:
        starts = torch.tensor(d["starts"], dtype=torch.long)
        kept = torch.clamp(y_lengths, max=out_size)
        col = torch.arange(out_size)
        src = (starts.unsqueeze(1) + col.unsqueeze(0)).clamp(max=frames - 1)
        live = (col.unsqueeze(0) < kept.unsqueeze(1)).unsqueeze(1)
        y = torch.gather(y, 2, src.unsqueeze(1).expand(-1, y.shape[1], -1)) * live.to(y.dtype)
        attn = torch.gather(attn, 2, src.unsqueeze(1).expand(-1, attn.shape[1], -1)) * live.to(attn.dtype)
        y_mask = U.sequence_mask(kept).unsqueeze(1).to(y_mask)
    mu_y = torch.matmul(attn.transpose(1, 2), mu_x.transpose(1, 2)).transpose(1, 2)
    nll = 0.5 * ((y - mu_y) ** 2 + math.log(2 * math.pi)) * y_mask
    prior_loss = nll.sum() / (y_mask.sum() * c.F)
    (G_DUR * dur_loss + G_PRIOR * prior_loss + (d["g_mu_y"].to(dtype) * mu_y).sum()).backward()
    return dict(y_c=y.detach(), mu_y=mu_y.detach(), dur_loss=dur_loss.detach(), prior_loss=prior_loss.detach(), dlogw=logw.grad,
                dmu_x=mu_x.grad)


def c_index(d):
    """(idx [B,T] int32, dur [B,t_x] fp32, first [B,t_x] int32) of the 0/1 path."""
    p = d["path"]
    idx = torch.where(p.sum(1) > 0, p.argmax(1), torch.full((), -1, dtype=torch.long)).to(torch.int32)
    dur = p.sum(-1)
    first = torch.where(dur > 0, p.argmax(2), torch.full((), -1, dtype=torch.long)).to(torch.int32)
    return idx, dur, first


def c_manual(c, d, mistake=None):
    """What the kernels compute, in float64: the index form of the path, the gather, both losses with their fixed normalisers, and the
    segment sum dmu_x[b,f,i] = sum over the live output frames c of token i of (g_mu_y + G_PRIOR inv_denom (mu_y - y_c))."""
    idx, dur, first = c_index(d)
    B, Fd, tx, T, S = c.B, c.F, c.tx, c.T, d["S"]
    kept = c_kept(c, d).tolist()
    starts = d["starts"]
    y, mu_x, g_mu_y = d["y"].double(), d["mu_x"].double(), d["g_mu_y"].double()
    x_mask, logw = d["x_mask"].double(), d["logw"].double()
    r = logw - torch.log(1e-8 + dur.double()).unsqueeze(1) * x_mask
    inv_d = 1.0 / float(d["x_lengths"].sum())
    out = dict(idx=idx, dur=dur, first=first, dur_loss=(r * r).sum() * inv_d, dlogw=G_DUR * 2.0 * r * inv_d)
    y_c = torch.zeros(B, Fd, S, dtype=torch.float64)
    mu_y = torch.zeros(B, Fd, S, dtype=torch.float64)
    total = 0.0
    for b in range(B):
        ncol = S if mistake == "live_mask_dropped" else kept[b]
        for col in range(ncol):
            src = min(starts[b] + col, T - 1)
            y_c[b, :, col] = y[b, :, src]
            if idx[b, src] >= 0:
                mu_y[b, :, col] = mu_x[b, :, idx[b, src]]
        total = total + (0.5 * ((y_c[b, :, :ncol] - mu_y[b, :, :ncol]) ** 2 + LOG_2PI)).sum()
    norm = float(d["y_lengths"].sum()) if mistake == "prior_normaliser_uncropped" else float(sum(kept))
    inv_p = 1.0 / (norm * Fd)
    dmu_x = torch.zeros(B, Fd, tx, dtype=torch.float64)
    for b in range(B):
        st = 0 if mistake == "start_taken_as_zero" else starts[b]
        for i in range(tx):
            if first[b, i] < 0:
                continue
            c0 = max(int(first[b, i]) - st, 0)
            c1 = min(int(first[b, i]) + int(dur[b, i]) - st + (1 if mistake == "segment_off_by_one" else 0), kept[b])
            if c1 > c0:
                dmu_x[b, :, i] = (g_mu_y[b, :, c0:c1] + G_PRIOR * inv_p * (mu_y[b, :, c0:c1] - y_c[b, :, c0:c1])).sum(-1)
    out.update(y_c=y_c, mu_y=mu_y, prior_loss=total * inv_p, dmu_x=dmu_x)
    return out


# mistake -> the op family it is restated on
MISTAKES = {"segment_off_by_one": "C", "live_mask_dropped": "C", "start_taken_as_zero": "C", "prior_normaliser_uncropped": "C",
            "taps_not_flipped": "A", "column_mask_dropped": "A", "decay_swapped": "B"}
