"""Catalogue of single-op cases of the encoders' two fp32 VALU kernels (csrc/enc.hip) -- enc_layernorm_kernel and the windowed
relative-position attention in its 8-query (enc_attention_kernel) and 16-query (enc_attention16_kernel) forms -- and their float64
references (oracle/encoder_oracle.py: layer_norm with its flags, attention_core with the reference's pad / reshape re-indexing).

tests/test_gpu_enc_ops.py runs every case on the GPU through gtts_enc_layernorm / gtts_enc_attention, the launches gtts_enc_forward
makes; tests/test_enc_op_cases_cpu.py proves without a GPU which kernel each case reaches, that each score regime is what its name
says, and that the GPU bound tells restated kernel mistakes from the kernel.

Error measure, per case:  e = max |got - ref64| / max |ref64| over ALL elements.  GPU bound:  e <= 4 e_ref32 + 2e-6 and e <= 1e-5,
e_ref32 = the same op in fp32 torch on the CPU (asserted <= 2e-6 for every case).

Score regimes of the attention cases (defined on the float64 scores, asserted by the CPU test):
  init       q, k, v are the 1x1 convolutions of oracle.encoder_oracle.make_state on unit-variance activations: scores with a standard
             deviation of ~0.3, an almost uniform softmax -- the only regime the whole-encoder tests ever ran
  peaked     keys of norm sqrt(dk); query i = T_i k_pi(i) / sqrt(dk), so that its score at key pi(i) is T_i = 12 (70 % of the rows) or
             4, and |score| <= T_i everywhere else (Cauchy-Schwarz) before the relative-key term: at least half the valid rows have
             max_j p_ij >= 0.9 and max |score| <= 30.  pi(i) lies inside the window for half of the rows, so the relative-value
             term carries the row's probability mass there
  saturated  the same with T_i = 400: in some rows the runner-up is more than 100 nats below the maximum and expf must give 0.
             Head widths >= 48 only: at dk = 4 two of 130 unit keys are often closer than 14 degrees, such a row's two leading
             scores differ by a few nats at a magnitude of 400, where one fp32 rounding of a score (2.4e-5) moves the probabilities by
             more than the bound -- in the fp32 reference as much as in the kernel.  That measures the conditioning of the row, not the
             kernel
Padded positions (t >= the item's length) hold values only the mask removes: q and k 100 times their valid scale, v four to eight
times its scale with alternating sign along t -- each padded v is large where a single one leaks into a row, while their sum over t
stays below one element, so that the rows of padded queries and of the fully masked item (every score -1e4: uniform over all L keys,
padded ones included) do not inflate max |ref64|, the normaliser of the error measure."""
import collections
import math

import torch

from case_util import relerr, seq_mask as _mask  # noqa: F401
from oracle import encoder_oracle as E

ELEMENTWISE_ABS = 2e-6          # the project's fp32 elementwise rule: e <= 4 e_ref32 + 2e-6 (test_gpu_spk.py, test_gpu_op_parity.py)
REDUCTION_REL = 1e-5            # the project's bound for fp32 reductions (SCALE_SHIFT; GroupNorm / Mish forward)
E32_MAX = 2e-6                  # what the fp32 torch restatement itself may lose against float64
LDS = 160 * 1024


def bound(e32):
    return min(4.0 * e32 + ELEMENTWISE_ABS, REDUCTION_REL)


def exceeds(e, b):
    return not (e <= b)          # a NaN exceeds every bound


# =============================================================================================================== attention
AttCase = collections.namedtuple("AttCase", "id B heads dk L window regime lens paths")


def lds16(dk, L):
    return (dk * 16 + 16 * 16 + 16 * ((L + 63) // 64 * 64) + 4 * 64) * 4


def lds8(dk, L):
    return (8 * dk + 8 * L) * 4


def eligible_paths(dk, window, L):
    p = []
    if lds8(dk, L) <= LDS:
        p.append(8)
    if dk % 4 == 0 and window <= 7 and lds16(dk, L) <= LDS:
        p.append(16)
    return tuple(p)


def _ragged(L, B):
    """B <= 3 lengths: the full one, about half, and a length-1 item (even L) or a fully masked one (odd L)."""
    return (L, max(1, L // 2), 1 if L % 2 == 0 else 0)[:B]


def att_case(tag, heads, dk, L, window, regime, B=3, lens=None, paths=None):
    lens = tuple(lens) if lens is not None else _ragged(L, B)
    assert len(lens) == B and max(lens) <= L
    paths = tuple(paths) if paths is not None else eligible_paths(dk, window, L)
    cid = "att-%s-h%d-dk%d-L%d-w%d-%s" % (tag, heads, dk, L, window, regime)
    return AttCase(cid, B, heads, dk, L, window, regime, lens, paths)


LENGTHS = (1, 3, 5, 9, 16, 17, 63, 64, 65, 130)      # below / at / beyond the window, the 8- and 16-query tiles, the 64-key block


def _att_cases():
    c = []
    # ---- every length, 2 heads of 48 channels, window 4
    for L in LENGTHS:
        c.append(att_case("len", 2, 48, L, 4, "init"))
        c.append(att_case("len", 2, 48, L, 4, "peaked"))
    for L in (5, 17, 64, 65, 130):
        c.append(att_case("len", 2, 48, L, 4, "saturated"))
    # ---- head widths and head counts (dk = 10: the 16-query kernel reads its queries as float4, path 8 only)
    # (peaked rows need keys that are far apart: 65 keys on the unit sphere of R^10, or 17 on that of R^4, are not, so dk = 10 is
    # peaked at L = 17 only and dk = 4 runs the init regime alone)
    for heads, dk in ((1, 4), (8, 4), (1, 10), (8, 10), (8, 48), (1, 96), (2, 96)):
        for L in (17, 65):
            c.append(att_case("width", heads, dk, L, 4, "init", B=2, lens=(L, L // 3)))
            if dk >= 48 or (dk == 10 and L == 17):
                c.append(att_case("width", heads, dk, L, 4, "peaked", B=2, lens=(L, L // 3)))
    c.append(att_case("width", 2, 96, 65, 4, "saturated", B=2, lens=(65, 21)))
    # ---- windows: none, the smallest, the 16-query kernel's last (15 of its 16 relative slots), one past it (path 8 only), and
    # windows larger than the sequence
    for window in (0, 1, 7, 8):
        c.append(att_case("win", 2, 48, 17, window, "init", B=2, lens=(17, 6)))
        c.append(att_case("win", 2, 48, 17, window, "peaked", B=2, lens=(17, 6)))
    for window in (4, 7, 8):
        c.append(att_case("win-gt-len", 2, 48, 3, window, "init", B=2, lens=(3, 2)))
    c.append(att_case("win-gt-len", 1, 4, 5, 7, "init", B=3, lens=(5, 1, 0)))
    c.append(att_case("win-gt-len", 2, 48, 5, 7, "peaked", B=3, lens=(5, 1, 0)))
    # ---- the last length of each kernel: both fill the 160 KB of LDS exactly (one head of 96 channels, B = 1)
    c.append(att_case("limit", 1, 96, 2432, 4, "init", B=1, lens=(2427,), paths=(16,)))
    c.append(att_case("limit", 1, 96, 5024, 4, "init", B=1, lens=(5019,), paths=(8,)))
    return c


ATT_CASES = _att_cases()
ATT_BY_ID = {c.id: c for c in ATT_CASES}
ATT_SMALL = [c for c in ATT_CASES if c.L <= 130]           # the cases the restated mistakes are evaluated on
T_PEAK, T_SOFT, T_SAT = 12.0, 4.0, 400.0


def att_inputs(c):
    """CPU fp32 tensors of one case: q, k, v [B, C, L], mask [B, L], ek, ev [2w+1, dk] (None without a window)."""
    g = torch.Generator().manual_seed(5000 + ATT_CASES.index(c))
    B, H, dk, L, w = c.B, c.heads, c.dk, c.L, c.window
    C = H * dk
    mask = _mask(c.lens, L)
    sd = E.make_state("mel", n_feats=4, C=C, filt=C, n_heads=H, n_layers=1, window=max(w, 1), seed=300 + ATT_CASES.index(c))
    p = "encoder.attn_layers.0."
    if c.regime == "init":
        x = torch.randn(B, C, L, generator=g) * mask.unsqueeze(1)
        q, k, v = (E.conv(sd, p + n, x, 1) for n in ("conv_q.", "conv_k.", "conv_v."))
    else:
        k = torch.randn(B, H, dk, L, generator=g)
        k = k / k.norm(dim=2, keepdim=True) * math.sqrt(dk)
        q = torch.empty(B, H, dk, L)
        for b in range(B):
            n = max(c.lens[b], 1)
            for h in range(H):
                near = (torch.arange(L) + torch.randint(-w - 1, w + 2, (L,), generator=g)).clamp(0, n - 1)
                far = torch.randint(0, n, (L,), generator=g)
                pi = torch.where(torch.rand(L, generator=g) < 0.5, near, far)
                if c.regime == "peaked":
                    T = torch.where(torch.rand(L, generator=g) < 0.7, torch.tensor(T_PEAK), torch.tensor(T_SOFT))
                else:
                    T = torch.full((L,), T_SAT)
                q[b, h] = k[b, h][:, pi] * (T / math.sqrt(dk)).unsqueeze(0)
        q, k = q.reshape(B, C, L), k.reshape(B, C, L)
        v = torch.randn(B, C, L, generator=g)
    # padded positions: large finite values that only the mask removes (see the module docstring)
    pad = (mask == 0).unsqueeze(1)
    sq, sk, sv = float(q.std()), float(k.std()), float(v.std())
    q = torch.where(pad, 100.0 * sq * torch.randn(B, C, L, generator=g), q)
    k = torch.where(pad, 100.0 * sk * torch.randn(B, C, L, generator=g), k)
    alt = (1.0 - 2.0 * (torch.arange(L) % 2)).view(1, 1, L) * (4.0 * sv * (1.0 + torch.rand(1, C, 1, generator=g)))
    v = torch.where(pad, alt.expand(B, C, L), v)
    d = dict(q=q.contiguous(), k=k.contiguous(), v=v.contiguous(), mask=mask, ek=None, ev=None)
    if w:
        d["ek"], d["ev"] = sd[p + "emb_rel_k"][0].contiguous(), sd[p + "emb_rel_v"][0].contiguous()
    return d


def att_slice(d, b):
    """Item b of a case alone, as a batch of one."""
    return dict(d, q=d["q"][b:b + 1].contiguous(), k=d["k"][b:b + 1].contiguous(), v=d["v"][b:b + 1].contiguous(),
                mask=d["mask"][b:b + 1].contiguous())


def att_reference(c, d, dtype=torch.float64):
    """oracle.encoder_oracle.attention_core (the reference's pad / reshape indexing) in `dtype`."""
    t = lambda x: None if x is None else x.to(dtype)
    m = t(d["mask"]).unsqueeze(1)
    attn_mask = m.unsqueeze(2) * m.unsqueeze(-1)
    ek = None if d["ek"] is None else t(d["ek"]).unsqueeze(0)
    ev = None if d["ev"] is None else t(d["ev"]).unsqueeze(0)
    return E.attention_core(t(d["q"]), t(d["k"]), t(d["v"]), attn_mask, ek, ev, c.heads, c.window)


ATT_MISTAKES = ("rel-index+1", "rel-index-1", "window-strict", "no-rel-v", "rel-k-unscaled", "no-key-mask", "no-query-mask",
                "head-offset", "softmax32-no-max")


def att_direct(c, d, mistake=None, want="out"):
    """The same attention with the kernels' direct index r = j - i + w into the 2w+1 embeddings, in float64 -- a second, independent
    indexing (the CPU test holds it to attention_core at 1e-12) on which the kernel mistakes of ATT_MISTAKES are restated.
    want = 'scores': the float64 scores after the mask fill [B, H, L, L]."""
    assert mistake is None or mistake in ATT_MISTAKES
    B, H, dk, L, w = c.B, c.heads, c.dk, c.L, c.window
    f = lambda x: x.double().view(B, H, dk, L).transpose(2, 3)                    # [B, H, L, dk]
    q, k, v = f(d["q"]), f(d["k"]), f(d["v"])
    scores = q @ k.transpose(-2, -1) / math.sqrt(dk)
    ii, jj = torch.meshgrid(torch.arange(L), torch.arange(L), indexing="ij")
    if w:
        nr = 2 * w + 1
        shift = {"rel-index+1": 1, "rel-index-1": -1}.get(mistake, 0)
        r = jj - ii + w + shift
        inside = (r >= 0) & (r < nr) & (((jj - ii).abs() < w) if mistake == "window-strict" else ((jj - ii).abs() <= w))
        rc = r.clamp(0, nr - 1)

        def emb(e):                                                               # [H, 2w+1, dk]: the same rows for every head
            e = e.double()
            if mistake == "head-offset":                                          # head h starts h rows into the table
                flat = e.flatten()
                return torch.stack([flat[(torch.arange(nr * dk) + h * nr * dk // 2 + h * dk) % (nr * dk)].view(nr, dk) for h in range(H)])
            return e.unsqueeze(0).expand(H, nr, dk)
        ek, ev = emb(d["ek"]), emb(d["ev"])
        rel = torch.einsum("bhid,hrd->bhir", q, ek)                               # q_i . Ek[r]
        rel = rel.gather(-1, rc.view(1, 1, L, L).expand(B, H, L, L)) * inside
        scores = scores + (rel if mistake == "rel-k-unscaled" else rel / math.sqrt(dk))
    m = d["mask"].double()
    mi, mj = m.view(B, 1, L, 1), m.view(B, 1, 1, L)
    dead = {"no-key-mask": mi.expand(B, 1, L, L) == 0, "no-query-mask": mj.expand(B, 1, L, L) == 0}.get(mistake, mi * mj == 0)
    scores = scores.masked_fill(dead, -1e4)
    if want == "scores":
        return scores
    if mistake == "softmax32-no-max":
        ex = torch.exp(scores.float())
        p = (ex / ex.sum(-1, keepdim=True)).double()
    else:
        p = torch.softmax(scores, -1)
    out = p @ v
    if w and mistake != "no-rel-v":
        wv = ev[:, rc] * inside.view(1, L, L, 1)                                  # [H, L, L, dk]: Ev[j - i + w] inside the window
        out = out + torch.einsum("bhij,hijd->bhid", p, wv)
    return out.transpose(2, 3).contiguous().view(B, H * dk, L)


# Cases whose e_ref32 is att_serial_fp32 instead of fp32 torch.  enc_attention_kernel sums the L products p_ij v_j of an output element in
# one serial fmaf chain; torch's matmul sums in blocks.  At L = 5024 with an almost uniform softmax (every term ~1 / L of the result) the
# chain's rounding walk, ~sqrt(L) / 2 ulp of the running sum, is 4.0e-6 of max |ref| against 3.6e-7 for torch: measured on the GPU
# e = 4.02e-06 where 4 e_torch32 + 2e-6 = 3.56e-06, and the restatement in the kernel's order gives 4.017e-06 on the CPU.  The
# 16-query kernel (64 partial sums per element, folded by a butterfly) stays at 3.0e-07 at its own limit L = 2432.
SERIAL_SUM_CASES = ("att-limit-h1-dk96-L5024-w4-init",)
SERIAL_ROWS = 8                     # the restatement covers query 0 of every 8-query workgroup tile: rows are independent of each other


def att_serial_fp32(c, d, rows=None):
    """The 8-query kernel's own arithmetic order in fp32 on the CPU, for the queries `rows` (default: all): fmaf chains over d for
    the scores, a per-lane (64 lanes) running maximum and sum folded by a butterfly, and ONE serial fmaf chain over all L keys per
    output element.  Returns [B, C, len(rows)].  O(dk + L) torch calls on [len(rows), L] tensors."""
    B, H, dk, L, w = c.B, c.heads, c.dk, c.L, c.window
    I = torch.arange(L) if rows is None else torch.as_tensor(rows)
    n = I.numel()
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(dk), dtype=torch.float32))
    f = lambda x: x.float().view(B, H, dk, L)
    q, k, v = f(d["q"])[..., I], f(d["k"]), f(d["v"])
    fma = lambda a, b, acc: (a.double() * b.double() + acc.double()).float()       # one rounding, like fmaf

    def lanes(x, op):                                                             # x [..., L] -> per-lane serial fold, then butterfly
        nb = (L + 63) // 64
        pad = torch.full(x.shape[:-1] + (nb * 64 - L,), float("-inf") if op == "max" else 0.0)
        x = torch.cat([x, pad], -1).view(x.shape[:-1] + (nb, 64))
        acc = x[..., 0, :]
        for t in range(1, nb):
            acc = torch.maximum(acc, x[..., t, :]) if op == "max" else acc + x[..., t, :]
        for s in (32, 16, 8, 4, 2, 1):
            o = acc[..., torch.arange(64) ^ s]
            acc = torch.maximum(acc, o) if op == "max" else acc + o
        return acc[..., :1]
    acc = torch.zeros(B, H, n, L)
    for dd in range(dk):
        acc = fma(q[:, :, dd, :, None], k[:, :, dd, None, :], acc)
    sc = acc * inv
    ii, jj = I.view(n, 1), torch.arange(L).view(1, L)
    if w:
        r = (jj - ii + w).expand(n, L)
        inside = (r >= 0) & (r <= 2 * w)
        ar = torch.zeros(B, H, n, 2 * w + 1)
        for dd in range(dk):
            ar = fma(q[:, :, dd, :, None], d["ek"][None, None, None, :, dd], ar)
        rel = ar.gather(-1, r.clamp(0, 2 * w).view(1, 1, n, L).expand(B, H, n, L))
        sc = torch.where(inside, sc + rel * inv, sc)
    m = d["mask"]
    sc = torch.where((m[:, I].view(B, 1, n, 1) * m.view(B, 1, 1, L)) == 0, torch.tensor(-1e4), sc)
    ex = torch.exp(sc - lanes(sc, "max"))
    p = ex * (torch.tensor(1.0) / lanes(ex, "sum"))
    out = torch.zeros(B, H, dk, n)
    for j in range(L):
        out = fma(p[:, :, None, :, j], v[:, :, :, None, j], out)
    if w:
        for rr in range(2 * w + 1):
            j = I + rr - w
            ok = (j >= 0) & (j < L)
            pj = p.gather(-1, j.clamp(0, L - 1).view(1, 1, n, 1).expand(B, H, n, 1))[..., 0]
            new = fma(pj[:, :, None, :], d["ev"][rr].view(1, 1, dk, 1), out)
            out = torch.where(ok.view(1, 1, 1, n), new, out)
    return out.reshape(B, H * dk, n)


# =============================================================================================================== LayerNorm
LnCase = collections.namedtuple("LnCase", "id B C L lens bres a_mask out_mask relu_in relu_out data")
FLAGS = ("bres", "a_mask", "out_mask", "relu_in", "relu_out")
# the four call sites of gtts_enc_forward
SITES = {"prenet": dict(relu_out=True), "norm1": dict(a_mask=True, bres=True), "norm2": dict(bres=True), "durpred": dict(relu_in=True)}
EPS = 1e-4


def ln_case(tag, C, L, B=2, lens=None, data="normal", **flags):
    lens = tuple(lens) if lens is not None else (L, max(1, L // 2))[:B]
    f = {k: bool(flags.get(k, False)) for k in FLAGS}
    name = "".join(k[0] + k.split("_")[-1][0] for k in FLAGS if f[k]) or "plain"      # bb, am, om, ri, ro
    return LnCase("ln-%s-C%d-L%d-%s" % (tag, C, L, name), B, C, L, lens, f["bres"], f["a_mask"], f["out_mask"], f["relu_in"],
                  f["relu_out"], data)


def _ln_cases():
    c = []
    for bits in range(32):                                                     # all 32 flag combinations
        c.append(ln_case("flags", 20, 17, lens=(17, 6), **{k: bool(bits >> n & 1) for n, k in enumerate(FLAGS)}))
    for site, C in (("prenet", 192), ("norm1", 192), ("norm2", 192), ("durpred", 256)):     # the call sites at their real widths
        for L in (1, 15, 16, 17, 130):
            c.append(ln_case(site, C, L, **SITES[site]))
    for C in (1, 10, 16, 17, 80):                                              # idle channel lanes, a partial last step of the walk
        c.append(ln_case("chan", C, 17, a_mask=True, bres=True))
        c.append(ln_case("chan", C, 17, relu_in=True, relu_out=C > 1, out_mask=True))   # (C = 1: the output is beta, of either sign)
    c.append(ln_case("const", 20, 17, data="const"))
    c.append(ln_case("const", 20, 17, data="const", relu_out=True))
    c.append(ln_case("const", 192, 17, data="const", relu_out=True))
    c.append(ln_case("lowvar", 192, 17, data="lowvar"))
    c.append(ln_case("lowvar", 20, 17, data="lowvar", relu_out=True))
    c.append(ln_case("offset", 192, 17, data="offset"))
    c.append(ln_case("offset", 256, 130, data="offset", relu_in=True))
    c.append(ln_case("offset", 20, 17, data="offset", bres=True))
    return c


LN_CASES = _ln_cases()
LN_BY_ID = {c.id: c for c in LN_CASES}
# columns (b, t) of a 'const' case whose C inputs are all equal to a value with a short mantissa: the fp32 sum of C <= 192 copies is exact,
# the mean IS the value, every deviation is 0 and the output is exactly beta (max(beta, 0) with relu_out), in any summation order
CONST_COLUMNS = {(0, 3): 1.5, (0, 5): -0.75, (1, 0): 3.0, (0, 16): 0.0}
CONST_AWKWARD = ((1, 2), 0.3)      # 0.3 is not exact in fp32 and its sums round: this column is held to the bound like any other


def ln_inputs(c):
    """a, bres [B, C, L], gamma, beta [C] (make_state's LayerNorm scale: 1 +- 0.1, +- 0.1), masks [B, L] from the lengths; padded
    positions of `a` are 100 times larger than valid ones (only a_mask removes them; without it they are normalised like any column).
      normal   standard normal
      const    normal, with the columns of CONST_COLUMNS / CONST_AWKWARD constant over the channels
      lowvar   every column = m_t + sqrt(1e-5) * normal with |m_t| <= 0.05: the variance is a tenth of eps = 1e-4, which decides the
               result.  (The mean stays small on purpose: the rounding of a mean of size m, ~1e-7 m, is multiplied by
               rsqrt(eps) = 100 in ANY fp32 two-pass LayerNorm; mean >> std is the next kind's subject)
      offset   20 + normal: mean >> std, as behind a ReLU with a large bias -- what a one-pass variance E[x^2] - mean^2 cannot hold"""
    g = torch.Generator().manual_seed(9000 + LN_CASES.index(c))
    B, C, L = c.B, c.C, c.L
    a = torch.randn(B, C, L, generator=g)
    if c.data == "lowvar":
        a = (torch.rand(B, 1, L, generator=g) - 0.5) * 0.1 + math.sqrt(1e-5) * a
    elif c.data == "offset":
        a = 20.0 + a
    elif c.data == "const":
        for (b, t), val in list(CONST_COLUMNS.items()) + [CONST_AWKWARD]:
            a[b, :, t] = val
    mask = _mask(c.lens, L)
    if c.data == "normal":
        a = torch.where((mask == 0).unsqueeze(1), 100.0 * a, a)
    d = dict(a=a.contiguous(), bres=torch.randn(B, C, L, generator=g) if c.bres else None,
             gamma=1.0 + 0.2 * (torch.rand(C, generator=g) - 0.5), beta=0.2 * (torch.rand(C, generator=g) - 0.5),
             a_mask=mask if c.a_mask else None, out_mask=mask if c.out_mask else None)
    return d


def ln_slice(d, b):
    cut = lambda x: None if x is None else x[b:b + 1].contiguous()
    return dict(d, a=cut(d["a"]), bres=cut(d["bres"]), a_mask=cut(d["a_mask"]), out_mask=cut(d["out_mask"]))


LN_MISTAKES = ("one-pass-fp32", "unbiased", "eps-1e-5", "relu-after", "mask-on-bres", "no-relu-out", "no-out-mask")


def ln_reference(c, d, dtype=torch.float64, mistake=None):
    """oracle.encoder_oracle.layer_norm with the case's flags in `dtype`; `mistake` restates one of LN_MISTAKES (None where the
    mistake cannot touch the case)."""
    assert mistake is None or mistake in LN_MISTAKES
    t = lambda x: None if x is None else x.to(dtype)
    um = lambda x: None if x is None else t(x).unsqueeze(1)
    sd = {"gamma": t(d["gamma"]), "beta": t(d["beta"])}
    a, bres, am, om = t(d["a"]), t(d["bres"]), um(d["a_mask"]), um(d["out_mask"])
    if mistake is None:
        return E.layer_norm(sd, "", a, EPS, bres=bres, a_mask=am, out_mask=om, relu_in=c.relu_in, relu_out=c.relu_out)
    eps, relu_out = EPS, c.relu_out
    x = a
    if mistake == "relu-after":                                    # ReLU behind the mask and the residual instead of before them
        if not (c.relu_in and c.bres):                             # (relu(a * mask) = relu(a) * mask for a 0 / 1 mask)
            return None
        x = x * am if c.a_mask else x
        x = x + bres if c.bres else x
        x = torch.relu(x)
    elif mistake == "mask-on-bres":
        if not (c.a_mask and c.bres) or c.out_mask or min(c.lens) == c.L or c.C == 1:    # (shows on padded columns of the output)
            return None
        x = (torch.relu(x) if c.relu_in else x)
        x = (x + bres) * am
    else:
        x = torch.relu(x) if c.relu_in else x
        x = x * am if c.a_mask else x
        x = x + bres if c.bres else x
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    if mistake == "one-pass-fp32":
        x32 = x.float()
        m32 = x32.mean(1, keepdim=True)
        mean, var = m32.to(dtype), ((x32 * x32).mean(1, keepdim=True) - m32 * m32).to(dtype)
    elif mistake == "unbiased":
        if c.C == 1:
            return None
        var = var * c.C / (c.C - 1)
    elif mistake == "eps-1e-5":
        eps = 1e-5
    elif mistake == "no-relu-out":
        if not c.relu_out:
            return None
        relu_out = False
    elif mistake == "no-out-mask":
        if not c.out_mask:
            return None
        om = None
    y = (x - mean) * torch.rsqrt(var + eps) * sd["gamma"].view(1, -1, 1) + sd["beta"].view(1, -1, 1)
    y = torch.relu(y) if relu_out else y
    return y * om if om is not None else y
