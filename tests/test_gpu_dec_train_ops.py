"""GPU parity tests (-m gpu) of the decoder's training kernels that are no convolution, one op at a time through the wrappers of _lib.py:
gn_mish_forward / _backward, in_glu_forward / _backward, attn_train_forward / _backward, rezero_forward / _backward, diffusion_noising,
score_loss.  The catalogue is tests/dec_train_op_cases.py; tests/test_dec_train_op_cases_cpu.py proves its restatements and that the
bound below tells restated mistakes from the kernels' contract.

  error     per tensor against float64 autograd of the plain torch expression, each in the norm the catalogue states (max |got - ref| /
            max |ref|; means over max |y|; rstd and 1 / S element-wise relative; dk over the scale of its two cancelling terms)
  bound     e <= 4 e_ref32 + 2e-6 and e <= 1e-5 (forward) / 1e-4 (gradients); the softmax row maximum exactly; dg of a random-sign dy
            within 1e-5 |dy| |f|
  guards    every input lies inside a larger allocation whose margins hold NaN, every output inside one filled with a sentinel; the
            margins must survive, every element must be written, every value finite
  repeats   each forward + backward is made twice and gives the same bits
Run with -s for the table (profiles/dec_train_op_parity.txt)."""
import functools
import importlib

import pytest
import torch

import dec_train_op_cases as D

pytestmark = pytest.mark.gpu
SENTINEL = -12345.675
NAN = float("nan")
MARGIN = 1024
F32 = torch.float32


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    return importlib.import_module("speech-backbones_amd")._lib


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def guarded(t, dev):
    """A contiguous device copy of t in the middle of a larger allocation whose margins hold NaN."""
    whole = torch.full((t.numel() + 2 * MARGIN,), NAN, dtype=F32, device=dev)
    view = whole[MARGIN:MARGIN + t.numel()].view(t.shape)
    view.copy_(t)
    return view


class Outputs:
    """Sentinel-filled, guarded fp32 output tensors by name; `collect` checks the margins, that every element was written and is
    finite, and returns CPU copies.  `head`: {name: n} -- only the first n floats of that tensor are values (behind them lies reduction
    scratch of another type, which is only checked to be written)."""

    def __init__(self, shapes, dev, head=None):
        self.t, self.head = {}, head or {}
        for n, shape in shapes.items():
            numel = 1
            for s in shape:
                numel *= s
            whole = torch.full((numel + 2 * MARGIN,), SENTINEL, dtype=F32, device=dev)
            self.t[n] = (whole[MARGIN:MARGIN + numel].view(shape), whole)

    def views(self):
        return {n: v[0] for n, v in self.t.items()}

    def collect(self):
        torch.cuda.synchronize()
        got = {}
        sent = torch.tensor(SENTINEL, dtype=F32)
        for n, (view, whole) in self.t.items():
            w, k = whole.cpu(), view.numel()
            assert bool((w[:MARGIN] == sent).all()) and bool((w[MARGIN + k:] == sent).all()), "a write outside %s" % n
            got[n] = w[MARGIN:MARGIN + k].view(view.shape).clone()
            bits = got[n].view(torch.int32)
            assert not bool((bits == sent.view(torch.int32)).any()), "an element of %s was never written" % n
            vals = got[n][:self.head[n]] if n in self.head else got[n]
            assert bool(torch.isfinite(vals).all()), "non-finite %s (a read outside an input)" % n
        return got


def same_bits(a, b):
    return all(torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)) for n in a)


@functools.lru_cache(maxsize=None)
def refs(fam, cid):
    """(case, inputs, float64 reference, e_ref32 per tensor): computed once per process, never modified."""
    cases, inputs, reference, _, _ = D.FAMILIES[fam]
    c = next(k for k in cases if k.id == cid)
    d = inputs(c)
    ref = reference(c, d)
    return c, d, ref, D.errors(fam, reference(c, d, torch.float32), ref)


_HEADER = []


def check(fam, c, got, ref, e32):
    """Print one table row per tensor and assert the bound of every held one."""
    if not _HEADER:
        _HEADER.append(1)
        print("\n%-40s %-9s %10s %9s %9s %9s" % ("case", "tensor", "max|ref|", "e", "e_ref32", "bound"))
    kind, fails = D.kind_of(fam, c), []
    for n, e in D.errors(fam, got, ref).items():
        is_held = D.is_held(fam, kind, n)
        b = "exact" if n == "stat_max" else "%9.2e" % (D.CS_REL if n == "dg_cs" else D.bound(e32[n], n))
        print("%-40s %-9s %10.3e %9.2e %9.2e %9s" % (c.id, n, float(ref[n].abs().max()), e, e32[n], b if is_held else "(unheld)"))
        if is_held and not D.passes(n, e, e32[n]):
            fails.append((n, e, e32[n]))
    assert not fails, (c.id, fails)


def twice(run):
    """run() -> dict of CPU tensors, made twice; the bits must repeat."""
    a, b = run(), run()
    assert same_bits(a, b), "the result differs between two calls on the same inputs"
    return a


@pytest.mark.parametrize("cid", [c.id for c in D.GN_CASES])
def test_groupnorm_mish_matches_float64(L, dev, cid):
    c, d, ref, e32 = refs("GN", cid)
    B, C, H, W, G = c.B, c.C, c.H, c.W, c.groups
    t = {n: guarded(d[n], dev) for n in ("y", "gamma", "beta", "mask", "dout")}
    tb = guarded(d["tb"], dev) if c.tb else None
    nst = int(L.lib().gtts_gn_mish_stats_floats(B, G))

    def run():
        o = Outputs(dict(out=(B, C, H, W), stats=(nst,)), dev, head=dict(stats=2 * B * G))
        out, stats = L.gn_mish_forward(t["y"], t["gamma"], t["beta"], t["mask"], G, D.EPS, tb=tb, out=o.views())
        assert out.data_ptr() == o.views()["out"].data_ptr() and stats.data_ptr() == o.views()["stats"].data_ptr()
        got = o.collect()
        shapes = dict(dy=(B, C, H, W), dgamma=(C,), dbeta=(C,))
        if c.tb:
            shapes["dtb"] = (B, C)
        ob = Outputs(shapes, dev)
        res = L.gn_mish_backward(t["dout"], t["y"], t["gamma"], t["beta"], t["mask"], stats, G, want_dtb=c.tb, out=ob.views())
        assert len(res) == (4 if c.tb else 3) and res[0].data_ptr() == ob.views()["dy"].data_ptr()
        got.update(ob.collect())
        return got

    got = twice(run)
    st = got["stats"][:2 * B * G].view(B, G, 2)
    got.update(mean=st[..., 0], rstd=st[..., 1])
    check("GN", c, got, ref, e32)
    # a masked column holds the time term alone (zero without one)
    dead = (d["mask"] == 0)[:, None, None, :].expand(B, C, H, W)
    want = d["tb"][:, :, None, None].expand(B, C, H, W) if c.tb else torch.zeros(B, C, H, W)
    assert torch.equal(got["out"][dead], want[dead])


@pytest.mark.parametrize("cid", [c.id for c in D.IN_CASES])
def test_instancenorm_glu_matches_float64(L, dev, cid):
    c, d, ref, e32 = refs("IN", cid)
    B, C, H, W = c.B, c.C, c.H, c.W
    t = {n: guarded(d[n], dev) for n in ("y", "gamma", "beta", "dout")}

    def run():
        o = Outputs(dict(out=(B, C, H, W), stats=(B * C * 4,)), dev)
        out, stats = L.in_glu_forward(t["y"], t["gamma"], t["beta"], D.EPS, out=o.views())
        assert out.data_ptr() == o.views()["out"].data_ptr() and stats.data_ptr() == o.views()["stats"].data_ptr()
        got = o.collect()
        ob = Outputs(dict(dy=(B, 2 * C, H, W), dgamma=(2 * C,), dbeta=(2 * C,)), dev)
        dy, _, _ = L.in_glu_backward(t["dout"], t["y"], t["gamma"], t["beta"], stats, out=ob.views())
        assert dy.data_ptr() == ob.views()["dy"].data_ptr()
        got.update(ob.collect())
        return got

    got = twice(run)
    st = got["stats"].view(B, C, 4)
    got.update(mean=st[..., 0::2], rstd=st[..., 1::2])
    check("IN", c, got, ref, e32)


@pytest.mark.parametrize("cid", [c.id for c in D.AT_CASES])
def test_linear_attention_core_matches_float64(L, dev, cid):
    c, d, ref, e32 = refs("AT", cid)
    B, C, N = D.AT_B, D.AT_HEADS * D.AT_D, c.N
    qkv, dout = guarded(d["qkv"], dev), guarded(d["dout"], dev)

    def run():
        o = Outputs(dict(out=(B, C, 1, N), ctx=(B, D.AT_HEADS, D.AT_D, D.AT_D), stat=(B, D.AT_HEADS, D.AT_D, 2)), dev)
        out, ctx, stat = L.attn_train_forward(qkv, out=o.views())
        assert out.data_ptr() == o.views()["out"].data_ptr() and ctx.data_ptr() == o.views()["ctx"].data_ptr()
        got = o.collect()
        ob = Outputs(dict(dqkv=(B, 3 * C, 1, N)), dev)
        dqkv = L.attn_train_backward(qkv, dout, ctx, stat, out=ob.views())
        assert dqkv.data_ptr() == ob.views()["dqkv"].data_ptr()
        got.update(ob.collect())
        return got

    got = twice(run)
    g = got["dqkv"]
    got.update(stat_max=got["stat"][..., 0], stat_inv=got["stat"][..., 1], dq=g[:, :C], dk=g[:, C:2 * C], dv=g[:, 2 * C:])
    check("AT", c, got, ref, e32)


@pytest.mark.parametrize("cid", [c.id for c in D.RZ_CASES])
def test_rezero_matches_float64(L, dev, cid):
    c, d, ref, e32 = refs("RZ", cid)
    t = {n: guarded(d[n], dev) for n in ("f", "x", "g", "dy")}

    def run():
        o = Outputs(dict(y=(c.n,)), dev)
        y = L.rezero_forward(t["f"], t["g"], t["x"], out=o.views())
        assert y.data_ptr() == o.views()["y"].data_ptr()
        got = o.collect()
        ob = Outputs(dict(df=(c.n,), dg=(1,)), dev)
        df, dg = L.rezero_backward(t["dy"], t["f"], t["g"], out=ob.views())
        assert df.data_ptr() == ob.views()["df"].data_ptr() and dg.data_ptr() == ob.views()["dg"].data_ptr()
        got.update(ob.collect())
        return got

    got = twice(run)
    if c.dy_kind == "random":
        got["dg_cs"] = got.pop("dg")
    check("RZ", c, got, ref, e32)


@pytest.mark.parametrize("cid", [c.id for c in D.NZ_CASES])
def test_noising_and_loss_head_match_float64(L, dev, cid):
    c, d, ref, e32 = refs("NZ", cid)
    t = {n: guarded(d[n], dev) for n in ("x0", "mu", "z", "mask", "t", "eps")}
    npart = int(L.lib().gtts_score_loss_partials(c.B, c.F, c.T))

    def run():
        o = Outputs(dict(xt=(c.B, c.F, c.T), zm=(c.B, c.F, c.T)), dev)
        xt, zm = L.diffusion_noising(t["x0"], t["mu"], t["z"], t["mask"], t["t"], D.BETA_MIN, D.BETA_MAX, out=o.views())
        assert xt.data_ptr() == o.views()["xt"].data_ptr() and zm.data_ptr() == o.views()["zm"].data_ptr()
        got = o.collect()
        ob = Outputs(dict(partials=(npart,), grad=(c.B, c.F, c.T)), dev)
        loss, geps = L.score_loss(t["eps"], zm, t["t"], D.BETA_MIN, D.BETA_MAX, d["inv_denom"], out=ob.views())
        assert geps.data_ptr() == ob.views()["grad"].data_ptr()
        got.update(ob.collect(), loss=loss.cpu().view(1))
        return got

    got = twice(run)
    got["geps"] = got["grad"]
    assert torch.equal(got["zm"], d["z"] * d["mask"][:, None])
    assert float(got["xt"][(d["mask"] == 0)[:, None].expand_as(got["xt"])].abs().max()) == 0.0
    check("NZ", c, got, ref, e32)
