"""GPU tests (-m gpu): every op of one estimator call, for every case of tests/op_parity_cases.py, against the same operation in float64 on
the CPU, evaluated on the HIP path's OWN input tensors of that op (the named intermediates of a keep_intermediates plan), so that a
producer's error is neither blamed on its consumer nor hidden by it.  tests/test_op_parity_cases_cpu.py proves without a GPU that the
catalogue launches every kernel instance of tests/golden/op_table.json and that every op label has exactly one checker.

States: O.make_estimator_state / V.make_state at their default rezero_g; inputs: O.make_inputs / V.make_inputs, seed 99, with the
catalogue's utterance lengths as the mask (DiffVC keeps the ragged ref_mask of V.make_inputs) and one t per utterance in both models.
Every float64 reference is asserted finite; nothing is skipped, and no element, op or utterance is left out of a comparison.  Errors
are max |got - ref| / max |ref| per op.

Check kinds (op_parity_cases.CLAIMS) and their references:
  stacked_input  x0 == stack(mu, x[, speaker plane]) / stack(mean, x, cond planes), copied exactly (bf16 storage: rounded to nearest
                 even exactly); spk_s against spk_mlp(spk) in float64
  time_bias      every tb row: ResnetBlock (and RefBlock) time projections, t_emb, DiffVC's sinusoidal embedding; the sin / cos argument
                 is the reference's fp32 product (scale * t) * freq, everything after it float64
  block_conv     conv2d(padding=1) of the masked input; b2: input (Mish(GroupNorm(b1.raw)) * mask + time bias) * mask with float64
                 statistics of b1.raw; concatenated inputs (up path) on both sources
  groupnorm      *.sc, *.sh against float64 mean / rstd of *.raw
  tail_identity  Mish(GN(b2.raw)) * mask + x * mask           res_tail   ... + res_conv(x * mask)
  downsample     conv2d(stride 2) of the masked attention output; where the level-0 attention output is folded into the Downsample's
                 weights (bf16x3 / f16f8) the op reads the attention's INPUT X, and the reference is that convolution of
                 (X + g * LinearAttention(X)) * mask, the attention in float64 (attention_f64 of tests/op_parity_cases.py)
  upsample       conv_transpose2d(stride 2, padding 1) of the masked input
  ref_conv       DiffVC RefBlock convolutions: input (GLU(InstanceNorm(prev.raw)) [+ time bias]) * ref_mask, float64 statistics
  instnorm       ref.blockNN.sc / .sh against float64 instance statistics (all positions, like InstanceNorm2d)
  ref_pool       the masked mean of GLU(IN(block32.raw)) over (mel bin, frame); the tensor holds the masked SUM, both sides are divided
                 by frames * mel bins
  cond           cond = cond_block(cat(sinusoidal embedding, RefBlock feature, c)) from the tb row, ref.pool and c
  final          the estimator output against final_conv(Mish(GN(final_block.raw)) * mask) * mask
  masked frames  every frame beyond an utterance's length is exactly 0 in the output of every identity tail and in the result -- where the
                 model defines it so (a 1x1 res_conv, a resampling convolution and an attention add their bias there: the float64 reference is
                 not 0 at those frames, and the comparison covers them like every other element)

Bounds (the project's existing ones):
  bf16x3 / f16f8 contractions   e <= 1e-4 (REL of tests/op_parity_cases.py); own error column: the same op in fp32 torch
  scale / shift                 e <= 1e-5
  elementwise fp32              e <= 4 e_ref32 + 2e-6 (tests/test_gpu_spk.py), e_ref32 the same op in float32 torch on the CPU
  bf16 / bf16_store             e <= 4 e_fmt (FMT_FACTOR of tests/op_parity_cases.py): e_fmt is the float64 reference with the contraction's
                                input (after its prologue, where the kernel rounds it) and weights rounded to bf16, bf16_store: the output
                                rounded too.  An elementwise op with a bf16 output: e_fmt is that output rounding.
  bf16, fp32 storage            in addition e_vs_fmt <= e_fmt: the kernel against the rounded-operand product itself must be nearer to it
                                than float64 is (fp32 accumulation and the rare operand that rounds to the other bf16 neighbour are all that
                                is left; Checker.contraction).  The format bound alone, 4 e_fmt = 1e-2 of max |ref|, passes a missing bias.
                                With bf16 storage the figure is printed only (a flipped output rounding is a whole ulp).
  bf16_store scale / shift      are reduced from the fp32 accumulators BEFORE the activations are rounded, which the stored tensor no longer
                                shows: bound 1e-5 + e_round, e_round the worst case over every fp32 tensor that rounds to the stored one
                                (2^-9 per element, propagated through mean and variance: gn_rounding_slack; about 2e-3, measured 5e-4).
                                For the same reason the consumers of a scale / shift (b2 convolution, tails, final) take the HIP path's
                                own *.sc / *.sh as the input they are with bf16 storage, where every other precision recomputes the
                                statistics from *.raw in float64.
Each op prints one row with -s: label, kernel instance (Plan.ops), shape, e_kernel, the reference's own error, the bound; the rows of a
whole case are printed before anything is asserted.  Figures: profiles/op_parity.txt."""
import math

import pytest
import torch
import torch.nn.functional as F

import op_parity_cases as C
from op_parity_cases import FMT_FACTOR, REL, RESNETS, _reader, attention_f64
from oracle import diffvc_oracle as V
from oracle import gradtts_oracle as O
from gpu_guards import S, dev  # noqa: F401

pytestmark = pytest.mark.gpu
SCALE_SHIFT = 1e-5
SEED = 99
T_VALUE = 0.7           # DiffVC: the t at which xt_ref was diffused; the estimator call itself gets one t per utterance, like Grad-TTS


# ------------------------------------------------------------------------------------------------ float64 / float32 operations
def _bf16(v):
    return v.float().to(torch.bfloat16).to(v.dtype)


def _maxrel(got, want):
    return float((got.double() - want.double()).abs().max() / (want.double().abs().max() + 1e-300))


def gn_scale_shift(raw, gamma, beta, groups=8):
    """[B, C] scale and shift of GroupNorm(groups, eps 1e-5, biased variance) in raw's dtype."""
    B, Cn = raw.shape[:2]
    g = raw.reshape(B, groups, -1)
    mean, rstd = g.mean(-1), 1.0 / torch.sqrt(g.var(-1, unbiased=False) + 1e-5)
    sc = gamma[None, :] * rstd.repeat_interleave(Cn // groups, 1)
    return sc, beta[None, :] - mean.repeat_interleave(Cn // groups, 1) * sc


def gn_rounding_slack(raw, gamma, groups=8):
    """Worst case of |scale - scale'|, |shift - shift'| ([B, C] each) between GroupNorm statistics of the stored bf16 tensor raw (scale,
    shift: gn_scale_shift) and of ANY fp32 tensor x that rounds to it, raw = x (1 + d), |d| <= u = 2^-9 per element:
    x = raw / (1 + d), so |x - raw| <= v |raw|, v = u / (1 - u), and |x^2 - raw^2| <= w raw^2, w = (1 - u)^-2 - 1.  With m, a, q the
    group means of raw, |raw|, raw^2:  |dmean| <= v a =: dm,  |dvar| <= w q + dm (2 |m| + dm) =: dv,
    |drstd| <= (var + eps - dv)^-1/2 - rstd,  |dscale| <= |gamma| |drstd|,  |dshift| <= dm (|scale| + |dscale|) + |m| |dscale|."""
    B, Cn = raw.shape[:2]
    u = 2.0 ** -9
    v, w = u / (1 - u), (1 - u) ** -2 - 1
    g = raw.reshape(B, groups, -1)
    m, a, q = g.mean(-1), g.abs().mean(-1), (g * g).mean(-1)
    var = g.var(-1, unbiased=False) + 1e-5
    dm = v * a
    dv = w * q + dm * (2 * m.abs() + dm)
    rstd = var ** -0.5
    per = lambda t: t.repeat_interleave(Cn // groups, 1)
    dsc = gamma.abs()[None, :] * per(torch.where(dv < var, (var - dv).clamp_min(1e-300) ** -0.5 - rstd, torch.full_like(var, math.inf)))      # (inf: no bound, the rounding could remove the whole variance)
    sc = gamma.abs()[None, :] * per(rstd)
    return dsc, per(dm) * (sc + dsc) + per(m.abs()) * dsc


def in_scale_shift(raw, gamma, beta):
    """[B, C] scale and shift of InstanceNorm2d(affine, eps 1e-5) over all positions."""
    B, Cn = raw.shape[:2]
    v = raw.reshape(B, Cn, -1)
    sc = gamma[None, :] / torch.sqrt(v.var(-1, unbiased=False) + 1e-5)
    return sc, beta[None, :] - v.mean(-1) * sc


def _norm(raw, sc, sh):
    return raw * sc[:, :, None, None] + sh[:, :, None, None]


def gn_mish(raw, gamma, beta):
    return O.mish(_norm(raw, *gn_scale_shift(raw, gamma, beta)))


def in_glu(raw, gamma, beta):
    return F.glu(_norm(raw, *in_scale_shift(raw, gamma, beta)), dim=1)


def time_rows(sd, t, dim, dt, vc):
    """(per-ResnetBlock / RefBlock time projections in program order, t_emb, sinusoidal embedding) in dtype dt."""
    half = dim // 2
    freq = torch.exp(torch.arange(half).float() * -(math.log(10000) / (half - 1)))       # the fp32 table, as Plan.pack builds it
    arg = ((1000.0 * t.float().unsqueeze(1)) * freq.unsqueeze(0)).to(dt)                 # the reference's fp32 products
    semb = torch.cat((arg.sin(), arg.cos()), -1)
    w = lambda n: sd[n].to(dt)
    t_emb = F.linear(O.mish(F.linear(semb, w("mlp.0.weight"), w("mlp.0.bias"))), w("mlp.2.weight"), w("mlp.2.bias"))
    names = (["ref_block.mlp1.1", "ref_block.mlp2.1"] if vc and "ref_block.mlp1.1.weight" in sd else []) + [n + ".mlp.1" for n in RESNETS]
    rows = [F.linear(O.mish(t_emb), w(n + ".weight"), w(n + ".bias")) for n in names]
    return names, rows, t_emb, semb


def mlp2(x, sd, p0, p2, dt):
    return F.linear(O.mish(F.linear(x.to(dt), sd[p0 + ".weight"].to(dt), sd[p0 + ".bias"].to(dt))), sd[p2 + ".weight"].to(dt), sd[p2 + ".bias"].to(dt))


# ------------------------------------------------------------------------------------------------ one case
class Checker:
    """Collects one table row per op and the failures of a case; nothing is asserted before every row is printed."""

    def __init__(self, case, kernels):
        self.case, self.kernels = case, kernels
        self.mode = {0: "split", 3: "split", 1: "bf16", 2: "store"}[case.prec]
        self.rows, self.failures, self.checked = [], [], set()

    def _row(self, label, what, shape, e, e_own, own, bound):
        ok = e <= bound
        self.rows.append("%-22s %-58s %-13s e_kernel %.2e %s %.2e bound %.2e%s" % (
            label + (" " + what if what else ""), self.kernels.get(label, "").replace("gtts::", ""), "x".join(str(v) for v in shape), e, own.strip(), e_own,
            bound, "" if ok else "  <-- FAILS"))
        if not ok:
            self.failures.append((label, what, e, bound))

    def _finite(self, label, ref):
        if not bool(torch.isfinite(ref).all()):
            self.failures.append((label, "the float64 reference is not finite"))

    def contraction(self, label, got, fn, x, w):
        """got against fn(x, w): fn is a contraction of x with w plus terms that depend on neither (a convolution with its bias, a 1x1
        res_conv on top of the elementwise half of a tail); x is the contraction's input after the prologue."""
        self.checked.add(label)
        ref = fn(x.double(), w.double())
        self._finite(label, ref)
        e = _maxrel(got, ref)
        if self.mode == "split":
            self._row(label, "", got.shape, e, _maxrel(fn(x.float(), w.float()), ref), "e_ref32", REL)
        else:
            fmt = fn(_bf16(x.double()), _bf16(w.double()))
            fmt = _bf16(fmt) if self.mode == "store" else fmt
            e_fmt = _maxrel(fmt, ref)
            self._row(label, "", got.shape, e, e_fmt, "e_fmt  ", FMT_FACTOR * e_fmt)
            # the kernel against the rounded-operand product itself.  fp32 storage: what is left is fp32 accumulation (K * 2^-24 against
            # e_fmt's 2^-9) and the operands whose fp32 prologue lies within fp32 error of a bf16 rounding boundary and rounds to the other
            # neighbour: one ulp at a fraction of about 2^-15 of the operands, where e_fmt is up to half an ulp at every one of them.  A
            # kernel that computes that product is therefore nearer to it than float64 is: e_vs_fmt <= e_fmt, asserted -- the format bound
            # alone passes an error of 4 e_fmt = 1e-2 of max |ref|, as large as a missing bias.  bf16 storage: a flipped OUTPUT rounding is
            # a whole ulp where e_fmt holds half a one, so the figure is printed only.
            e_vs = float((got.double() - fmt).abs().max() / ref.abs().max())
            bad = self.mode == "bf16" and not e_vs <= e_fmt
            self.rows[-1] += "  e_vs_fmt %.2e%s" % (e_vs, "  <-- FAILS (e_vs_fmt > e_fmt)" if bad else "")
            if bad:
                self.failures.append((label, "e_vs_fmt", e_vs, e_fmt))
        return ref

    def elementwise(self, label, got, fn, args, what="", bf16_out=False):
        """got against fn(*args) in float64; fn(*args) in float32 gives the float32 reference's own error."""
        self.checked.add(label)
        ref = fn(*[a.double() for a in args])
        self._finite(label, ref)
        e = _maxrel(got, ref)
        if bf16_out:
            e_fmt = _maxrel(_bf16(ref), ref)
            self._row(label, what, got.shape, e, e_fmt, "e_fmt  ", FMT_FACTOR * e_fmt)
        else:
            e32 = _maxrel(fn(*[a.float() for a in args]), ref)
            self._row(label, what, got.shape, e, e32, "e_ref32", 4 * e32 + 2e-6)
        return ref

    def scale_shift(self, label, got_sc, got_sh, sc, sh, slack=None):
        """slack: gn_rounding_slack of the stored tensor (bf16 storage only)."""
        self.checked.add(label)
        first = len(self.rows)
        for what, got, want, k in (("scale", got_sc, sc, 0), ("shift", got_sh, sh, 1)):
            self._finite(label, want)
            if slack is None:
                self._row(label, what, got.shape, _maxrel(got.view_as(want), want), 0.0, "-", SCALE_SHIFT)
            else:
                e_round = float(slack[k].max() / want.abs().max())
                self._row(label, what, got.shape, _maxrel(got.view_as(want), want), e_round, "e_round", SCALE_SHIFT + e_round)
        shift = self.rows.pop()                     # one printed row per op: scale, then the shift's figures
        self.rows[first] += " | shift" + shift[shift.index(" e_kernel"):]

    def exact(self, label, got, want, what):
        self.checked.add(label)
        same = torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))
        self._row(label, what, got.shape, 0.0 if same else _maxrel(got, want) + 1e-30, 0.0, "exact  ", 0.0)

    def zeros_beyond(self, label, got, ref, lengths, lvl):
        """Frames beyond an utterance's length: the reference is exactly 0 there (the assertion is not vacuous) and so is the kernel."""
        for b, L in enumerate(lengths):
            first = (L + (1 << lvl) - 1) >> lvl                    # mask[::2^lvl]: first column whose frame lies beyond the utterance
            if first < got.shape[-1]:
                if float(ref[b, ..., first:].abs().max()) != 0.0:
                    self.failures.append((label, "the reference is not 0 beyond the utterance", b))
                if not bool((got[b, ..., first:] == 0).all()):
                    self.failures.append((label, "not exactly 0 beyond utterance %d's length" % b))


def check_case(case, sd, a, get, out, kernels):
    """All op checks of one estimator call.  a: the call's CPU inputs; get: name -> CPU fp32 copy of a named intermediate."""
    ck = Checker(case, kernels)
    store, vc, dim = case.prec == 2, case.arch == 1, case.dim
    B, T = case.B, case.T
    m0 = a["mask"].view(B, 1, 1, T).double()
    masks = [m0, m0[..., ::2], m0[..., ::4]]
    D = lambda n: sd[n].double()
    folded = case.prec in (0, 3)                                   # plan.hip: level-0 attention output folded into downs.0.3 (C <= 256)

    # ---- time bias rows
    tb = get("tb").view(B, -1)
    names, _, _, _ = time_rows(sd, a["t"], dim, torch.float64, vc)

    def tb_fn(t):
        _, rows, t_emb, semb = time_rows(sd, a["t"], dim, t.dtype, vc)
        return torch.cat(rows + [t_emb] + ([semb] if vc else []), 1)
    want_tb = ck.elementwise("time_mlp", tb, tb_fn, [a["t"]])
    assert tb.shape == want_tb.shape, (tb.shape, want_tb.shape)
    tbcol, off = {}, 0
    for n in names:
        c = sd[n + ".weight"].shape[0]
        tbcol[n] = tb[:, off:off + c].double()
        off += c
    semb_hip = tb[:, off + dim: off + 2 * dim]

    # ---- DiffVC condition path
    if vc:
        Tr = case.T_ref
        if case.use_ref_t:
            rm = a["ref_mask"].view(B, 1, 1, Tr).double()
            ck.exact("ref.block11.conv", get("xt_ref"), a["xt_ref"], "xt_ref copy")
            prev, prev_name = a["xt_ref"].double(), None
            blocks = ("block11", "block12", "block21", "block22", "block31", "block32")
            for k, blk in enumerate(blocks):
                p = "ref_block.%s." % blk
                if k == 0:
                    xin = prev * rm
                else:
                    xin = in_glu(prev, D("ref_block.%s.1.weight" % prev_name), D("ref_block.%s.1.bias" % prev_name))
                    if blk in ("block21", "block31"):
                        xin = xin + tbcol["ref_block.mlp%d.1" % {"block21": 1, "block31": 2}[blk]][:, :, None, None]     # modules.py:162,164
                    xin = xin * rm
                raw = get("ref.%s.raw" % blk)
                ck.contraction("ref.%s.conv" % blk, raw, lambda x, w, p=p: F.conv2d(x, w, sd[p + "0.bias"].to(x.dtype), padding=1), xin, sd[p + "0.weight"])
                sc, sh = in_scale_shift(raw.double(), D(p + "1.weight"), D(p + "1.bias"))
                ck.scale_shift("ref.%s.in" % blk, get("ref.%s.sc" % blk).view(B, -1), get("ref.%s.sh" % blk).view(B, -1), sc, sh)
                prev, prev_name = raw.double(), blk
            rlen = a["ref_mask"].view(B, Tr).sum(-1).double()
            denom = (rlen * 80.0)[:, None]
            pool = get("ref.pool").view(B, -1)
            g32, b32 = sd["ref_block.block32.1.weight"], sd["ref_block.block32.1.bias"]
            ck.elementwise("ref.pool", pool.double() / denom,
                           lambda r, g, b, m: (in_glu(r, g, b) * m * m).sum((2, 3)) / denom.to(r.dtype), [prev, g32, b32, rm], "masked mean")

        def cond_fn(semb, c, *rest):
            parts = [semb]
            if case.use_ref_t:
                S_, fw, fb = rest
                L = (rlen * 80.0).to(semb.dtype)[:, None]
                parts.append((F.linear(S_, fw.view(fw.shape[0], -1)) + fb[None, :] * L) / L)
            return mlp2(torch.cat(parts + [c], 1), sd, "cond_block.0", "cond_block.2", semb.dtype)
        rest = [pool, sd["ref_block.final_conv.weight"], sd["ref_block.final_conv.bias"]] if case.use_ref_t else []
        cond = get("cond").view(B, -1)
        ck.elementwise("cond_block", cond, cond_fn, [semb_hip, a["c"]] + rest)

    # ---- stacked input
    x0 = get("x0")
    planes = [a["mu"], a["x"]]
    if vc:
        planes = [a["mu"], a["x"]] + [cond[:, j, None, None].expand(B, 80, T) for j in range(cond.shape[1])]
    elif case.n_spks > 1:
        s = get("spk_s").view(B, -1)
        ck.elementwise("spk_mlp", s, lambda v: mlp2(v, sd, "spk_mlp.0", "spk_mlp.2", v.dtype), [a["spk"]])
        planes.append(s[:, :, None].expand(B, 80, T))
    want_x0 = torch.stack(planes, 1).float()
    ck.exact("prep_input", x0, _bf16(want_x0) if store else want_x0, "x0 == stacked planes")

    # ---- the U-Net
    def conv3(bias):
        return lambda x, w: F.conv2d(x, w, sd[bias].to(x.dtype), padding=1)

    def gn_check(label, raw, p):
        sc, sh = gn_scale_shift(raw.double(), D(p + "block.1.weight"), D(p + "block.1.bias"))
        # bf16 storage: the statistics saw the fp32 accumulators; the stored tensor is rounded (module docstring)
        slack = gn_rounding_slack(raw.double(), D(p + "block.1.weight")) if store else None
        name = label[:-3]
        ck.scale_shift(label, get(name + ".sc").view(B, -1), get(name + ".sh").view(B, -1), sc, sh, slack)

    def act(raw, p0, p1):
        """Mish(GroupNorm(raw)): (p0, p1) = (gamma, beta), statistics of raw in its dtype; bf16 storage: the op's own (scale, shift)."""
        return O.mish(_norm(raw, p0, p1)) if store else gn_mish(raw, p0, p1)

    def norm_args(name, p):
        if store:       # reduced from the fp32 accumulators before the activations were rounded: not a function of the stored tensor
            return [get(name + ".sc").view(B, -1), get(name + ".sh").view(B, -1)]
        return [sd[p + "block.1.weight"], sd[p + "block.1.bias"]]

    def tail_fn(m):
        def fn(raw, x, p0, p1):
            mm = m.to(raw.dtype)
            return act(raw, p0, p1) * mm + x * mm
        return fn

    def resnet(name, xin, lvl):
        m, p = masks[lvl], name + "."
        b1 = get(name + ".b1.raw")
        ck.contraction(name + ".b1.conv", b1, conv3(p + "block1.block.0.bias"), xin.double() * m, sd[p + "block1.block.0.weight"])
        gn_check(name + ".b1.gn", b1, p + "block1.")
        h = (act(b1.double(), *[v.double() for v in norm_args(name + ".b1", p + "block1.")]) * m + tbcol[name + ".mlp.1"][:, :, None, None]) * m
        b2 = get(name + ".b2.raw")
        ck.contraction(name + ".b2.conv", b2, conv3(p + "block2.block.0.bias"), h, sd[p + "block2.block.0.weight"])
        gn_check(name + ".b2.gn", b2, p + "block2.")
        o = get(name + ".out")
        if (p + "res_conv.weight") in sd:
            # a 1x1 contraction in the epilogue on top of the elementwise GroupNorm / Mish half: the bound is the contraction's
            nargs = norm_args(name + ".b2", p + "block2.")

            def res_fn(xm, w):
                dt = xm.dtype
                h = act(b2.to(dt), *[v.to(dt) for v in nargs]) * m.to(dt)
                return h + F.conv2d(xm, w, sd[p + "res_conv.bias"].to(dt))
            ck.contraction(name + ".res_tail", o, res_fn, xin.double() * m, sd[p + "res_conv.weight"])
        else:
            args = [b2, xin] + norm_args(name + ".b2", p + "block2.")
            ref = ck.elementwise(name + ".tail", o, tail_fn(m), args, bf16_out=store)
            ck.zeros_beyond(name + ".tail", o, ref, case.lengths, lvl)
        return o

    def resample(name, xin, lvl, up):
        w, b = sd[name + ".conv.weight"], name + ".conv.bias"
        fn = (lambda x, w: F.conv_transpose2d(x, w, sd[b].to(x.dtype), stride=2, padding=1)) if up else \
             (lambda x, w: F.conv2d(x, w, sd[b].to(x.dtype), stride=2, padding=1))
        o = get(name + ".out")
        ck.contraction(name, o, fn, xin.double() * masks[lvl], w)
        return o

    x = x0
    hidden = []
    for lv in range(3):
        x = resnet("downs.%d.0" % lv, x, lv)
        x = resnet("downs.%d.1" % lv, x, lv)
        a_out = get("downs.%d.2.out" % lv)
        hidden.append(a_out)
        if lv < 2:
            if lv == 0 and folded:
                src = x.double() + attention_f64(sd, "downs.0.2", x)[1]
            else:
                src = a_out
            x = resample("downs.%d.3" % lv, src, lv, False)
        else:
            x = a_out
    x = resnet("mid_block1", x, 2)
    x = get("mid_attn.out")
    x = resnet("mid_block2", x, 2)
    for u in range(2):
        lv = 2 - u
        x = torch.cat((x, hidden.pop()), 1)
        x = resnet("ups.%d.0" % u, x, lv)
        x = resnet("ups.%d.1" % u, x, lv)
        x = resample("ups.%d.3" % u, get("ups.%d.2.out" % u), lv, True)
    fraw = get("final_block.raw")
    ck.contraction("final_block.conv", fraw, conv3("final_block.block.0.bias"), x.double() * m0, sd["final_block.block.0.weight"])
    gn_check("final_block.gn", fraw, "final_block.")

    def final_fn(raw, p0, p1, w, b):
        mm = m0.to(raw.dtype)
        return (F.conv2d(act(raw, p0, p1) * mm * mm, w, b) * mm).squeeze(1)
    ref = ck.elementwise("final_conv+euler", out, final_fn, [fraw] + norm_args("final_block", "final_block.") + [sd["final_conv.weight"], sd["final_conv.bias"]])
    ck.zeros_beyond("final_conv+euler", out.unsqueeze(1), ref.unsqueeze(1), case.lengths, 0)
    return ck


# ------------------------------------------------------------------------------------------------ states, plans, calls
_STATES, _PLANS = {}, {}


def state(case):
    key = (case.arch, case.dim, case.n_spks, case.use_ref_t)
    if key not in _STATES:
        if case.arch == 0:
            _STATES[key] = O.make_estimator_state(dim=case.dim, n_spks=case.n_spks, seed=5)
        else:
            _STATES[key] = V.make_state(dim_base=case.dim, dim_cond=128, use_ref_t=case.use_ref_t, seed=5)
    return _STATES[key]


def inputs(case):
    """CPU inputs of the estimator call of a case (shared names: x, mu, mask, t)."""
    B, T = case.B, case.T
    mask = O.sequence_mask(torch.tensor(case.lengths), T).unsqueeze(1).float()
    if case.arch == 0:
        inp = O.make_inputs(B, T, seed=SEED, spk_dim=64 if case.n_spks > 1 else None)
        return {"x": inp["z"], "mu": inp["mu"], "mask": mask, "t": torch.linspace(0.15, 0.9, B), "spk": inp.get("spk")}
    inp = V.make_inputs(B, T, case.T_ref, seed=SEED)
    xt_ref = torch.stack([V.compute_diffused_mean(inp["ref"], inp["ref_mask"], inp["mean_ref"], T_VALUE)], 1)
    return {"x": inp["z"], "mu": inp["mean"], "mask": mask, "t": torch.linspace(0.15, 0.9, B), "xt_ref": xt_ref, "ref_mask": inp["ref_mask"], "c": inp["c"]}


def _plan(S, dev, case):
    """keep_intermediates plan and its packed weights: one per configuration and process (the last one only: dim 256 packs 0.5 GB)."""
    kw = C.plan_kwargs(case)
    key = tuple(sorted(kw.items())) + (case.use_ref_t,)
    if key not in _PLANS:
        _PLANS.clear()
        plan = S.Plan(**kw)
        _PLANS[key] = (plan, plan.pack(state(case), dev))
    return _PLANS[key]


def run_case(S, dev, case):
    """One estimator call on the GPU; returns (inputs, reader of the named intermediates, result, {op label: kernel instance})."""
    plan, blob = _plan(S, dev, case)
    a = inputs(case)
    B, T = case.B, case.T
    g = lambda n: a[n].to(dev)
    if case.arch == 0:
        out = plan.estimator_forward(blob, g("x"), g("mask"), g("mu"), g("t"), g("spk") if case.n_spks > 1 else None)
        torch.cuda.synchronize()
        ws = plan.workspace(B, T, dev)
        infos = {n: (off, dims) for n, off, dims in plan._tensor_infos("gtts_plan_tensor_info", B, T)}
    else:
        out = plan.vc_estimator_forward(blob, g("x"), g("mask"), g("mu"), g("xt_ref"), g("ref_mask"), g("c"), g("t"))
        torch.cuda.synchronize()
        ws, infos = plan.vc_tensors(B, T, case.T_ref, dev)
    kernels = {}
    for label, kern, _, _ in plan.ops(B, T):
        if C.claims(case, label, kern)[0] not in C.NOT_CHECKED_HERE:
            kernels[label] = kern
    return a, _reader(ws, infos, case.prec == 2), out.cpu(), kernels


@pytest.mark.parametrize("case", C.CASES, ids=[c.id for c in C.CASES])
def test_every_op_against_float64_on_its_own_input(S, dev, case):
    a, get, out, kernels = run_case(S, dev, case)
    ck = check_case(case, state(case), a, get, out, kernels)
    print("\n==== %s" % case.id)
    for row in ck.rows:
        print(row)
    assert ck.checked == set(kernels), ("checked and claimed ops differ", sorted(ck.checked ^ set(kernels)))
    assert not ck.failures, ck.failures
