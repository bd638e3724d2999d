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

import pytest
import torch

import dec_train_op_cases as D
from gpu_guards import NAN, L, Outputs, dev, guarded, guarded_inputs, table_row, twice  # noqa: F401

pytestmark = pytest.mark.gpu
MARGIN = 1024


@functools.lru_cache(maxsize=None)
def refs(fam, cid):
    """(case, inputs, float64 reference, e_ref32 per tensor): computed once per process, never modified."""
    cases, inputs, reference, _, _ = D.FAMILIES[fam]
    c = next(k for k in cases if k.id == cid)
    d = inputs(c)
    ref = reference(c, d)
    return c, d, ref, D.errors(fam, reference(c, d, torch.float32), ref)


def check(fam, c, got, ref, e32):
    """Print one table row per tensor and assert the bound of every held one."""
    kind, fails = D.kind_of(fam, c), []
    for n, e in D.errors(fam, got, ref).items():
        is_held = D.is_held(fam, kind, n)
        b = "exact" if n == "stat_max" else "%9.2e" % (D.CS_REL if n == "dg_cs" else D.bound(e32[n], n))
        table_row(__name__, "\n%-40s %-9s %10s %9s %9s %9s" % ("case", "tensor", "max|ref|", "e", "e_ref32", "bound"),
                  "%-40s %-9s %10.3e %9.2e %9.2e %9s" % (c.id, n, float(ref[n].abs().max()), e, e32[n], b if is_held else "(unheld)"))
        if is_held and not D.passes(n, e, e32[n]):
            fails.append((n, e, e32[n]))
    assert not fails, (c.id, fails)


@pytest.mark.parametrize("cid", [c.id for c in D.GN_CASES])
def test_groupnorm_mish_matches_float64(L, dev, cid):
    c, d, ref, e32 = refs("GN", cid)
    B, C, H, W, G = c.B, c.C, c.H, c.W, c.groups
    t = guarded_inputs(d, ("y", "gamma", "beta", "mask", "dout"), MARGIN, dev)
    tb = guarded(d["tb"], MARGIN, NAN, dev)[0] if c.tb else None
    nst = int(L.lib().gtts_gn_mish_stats_floats(B, G))

    def run():
        o = Outputs(dev, MARGIN).with_results(dict(out=(B, C, H, W), stats=(nst,)))
        out, stats = L.gn_mish_forward(t["y"], t["gamma"], t["beta"], t["mask"], G, D.EPS, tb=tb, out=o.views())
        assert out.data_ptr() == o.views()["out"].data_ptr() and stats.data_ptr() == o.views()["stats"].data_ptr()
        got = o.collect(head=dict(stats=2 * B * G))
        shapes = dict(dy=(B, C, H, W), dgamma=(C,), dbeta=(C,))
        if c.tb:
            shapes["dtb"] = (B, C)
        ob = Outputs(dev, MARGIN).with_results(shapes)
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
    t = guarded_inputs(d, ("y", "gamma", "beta", "dout"), MARGIN, dev)

    def run():
        o = Outputs(dev, MARGIN).with_results(dict(out=(B, C, H, W), stats=(B * C * 4,)))
        out, stats = L.in_glu_forward(t["y"], t["gamma"], t["beta"], D.EPS, out=o.views())
        assert out.data_ptr() == o.views()["out"].data_ptr() and stats.data_ptr() == o.views()["stats"].data_ptr()
        got = o.collect()
        ob = Outputs(dev, MARGIN).with_results(dict(dy=(B, 2 * C, H, W), dgamma=(2 * C,), dbeta=(2 * C,)))
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
    qkv, dout = (guarded(d[n], MARGIN, NAN, dev)[0] for n in ("qkv", "dout"))

    def run():
        o = Outputs(dev, MARGIN).with_results(dict(out=(B, C, 1, N), ctx=(B, D.AT_HEADS, D.AT_D, D.AT_D), stat=(B, D.AT_HEADS, D.AT_D, 2)))
        out, ctx, stat = L.attn_train_forward(qkv, out=o.views())
        assert out.data_ptr() == o.views()["out"].data_ptr() and ctx.data_ptr() == o.views()["ctx"].data_ptr()
        got = o.collect()
        ob = Outputs(dev, MARGIN).with_results(dict(dqkv=(B, 3 * C, 1, N)))
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
    t = guarded_inputs(d, ("f", "x", "g", "dy"), MARGIN, dev)

    def run():
        o = Outputs(dev, MARGIN).with_results(dict(y=(c.n,)))
        y = L.rezero_forward(t["f"], t["g"], t["x"], out=o.views())
        assert y.data_ptr() == o.views()["y"].data_ptr()
        got = o.collect()
        ob = Outputs(dev, MARGIN).with_results(dict(df=(c.n,), dg=(1,)))
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
    t = guarded_inputs(d, ("x0", "mu", "z", "mask", "t", "eps"), MARGIN, dev)
    npart = int(L.lib().gtts_score_loss_partials(c.B, c.F, c.T))

    def run():
        o = Outputs(dev, MARGIN).with_results(dict(xt=(c.B, c.F, c.T), zm=(c.B, c.F, c.T)))
        xt, zm = L.diffusion_noising(t["x0"], t["mu"], t["z"], t["mask"], t["t"], D.BETA_MIN, D.BETA_MAX, out=o.views())
        assert xt.data_ptr() == o.views()["xt"].data_ptr() and zm.data_ptr() == o.views()["zm"].data_ptr()
        got = o.collect()
        ob = Outputs(dev, MARGIN).with_results(dict(partials=(npart,), grad=(c.B, c.F, c.T)))
        loss, geps = L.score_loss(t["eps"], zm, t["t"], D.BETA_MIN, D.BETA_MAX, d["inv_denom"], out=ob.views())
        assert geps.data_ptr() == ob.views()["grad"].data_ptr()
        got.update(ob.collect(), loss=loss.cpu().view(1))
        return got

    got = twice(run)
    got["geps"] = got["grad"]
    assert torch.equal(got["zm"], d["z"] * d["mask"][:, None])
    assert float(got["xt"][(d["mask"] == 0)[:, None].expand_as(got["xt"])].abs().max()) == 0.0
    check("NZ", c, got, ref, e32)
