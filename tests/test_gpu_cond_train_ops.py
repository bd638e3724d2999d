"""GPU parity tests (-m gpu) of the kernels of the DiffVC decoder's condition path under training, one op at a time through the ABI
wrappers of _lib.py: gtts_cond_field_forward / _backward, gtts_masked_mean_forward / _backward, gtts_in_glu_tb_forward / _backward
(in_glu_forward with tb, in_glu_backward with want_dtb),
gtts_conv3x3_narrow_forward / _dgrad / _wgrad.
The catalogue is tests/cond_train_cases.py; tests/test_cond_train_cases_cpu.py proves its restatements and that the bound below tells
restated mistakes from the kernels' contract.

  error     per tensor e = max |got - ref64| / max |ref64|, ref64 = float64 autograd of the torch composition on the kernel's own inputs
  bound     e <= 4 e_ref32 + 2e-6 and e <= 1e-4 (e_ref32: the same autograd in fp32 torch on the CPU), as tests/test_gpu_glue_train_ops.py;
            the integer-valued cases are compared with torch.equal
  guards    every input lies inside a larger allocation whose margins hold NaN, every output inside one filled with a sentinel
  repeats   every call is made twice and gives the same bits
Run with -s for the table."""
import functools

import pytest
import torch

import cond_train_cases as G
from gpu_guards import L, Outputs, dev, guarded_inputs, same_bits, table_row, twice  # noqa: F401

pytestmark = pytest.mark.gpu
MARGIN = 1024        # more than a row and a column of the widest plane (W = 130): a tap read one row outside a tensor lands in the margin


def held(cid, name, got, ref, r32, fails):
    e32, e = G.relerr(r32, ref), G.relerr(got, ref)
    table_row(__name__, "\n%-44s %-8s %10s %9s %9s %9s" % ("case", "tensor", "max|ref|", "e", "e_ref32", "bound"),
              "%-44s %-8s %10.3e %9.2e %9.2e %9.2e" % (cid, name, float(torch.as_tensor(ref).abs().max()), e, e32, G.bound(e32)))
    if not (e <= 4.0 * e32 + G.GRAD_ABS and e <= G.GRAD_REL):
        fails.append((name, e, e32))


@functools.lru_cache(maxsize=None)
def refs(fam, cid):
    """(case, inputs, float64 reference, fp32 reference): computed once per process, never modified."""
    cases, inputs, comp = {"F": (G.F_BY_ID, G.f_inputs, G.f_composition), "P": (G.P_BY_ID, G.p_inputs, G.p_composition),
                           "G": (G.G_BY_ID, G.g_inputs, G.g_composition)}[fam]
    c = cases[cid]
    d = inputs(c)
    return c, d, comp(c, d), comp(c, d, torch.float32)


@pytest.mark.parametrize("cid", [c.id for c in G.F_CASES])
def test_condition_field_matches_float64(L, dev, cid):
    c, d, ref, r32 = refs("F", cid)
    t = guarded_inputs(d, ("U", "base", "dy", "mask"), MARGIN, dev)

    def forward():
        o = Outputs(dev, MARGIN).with_results(dict(out=(c.B, c.C, c.H, c.W)))
        out = L.cond_field(t["U"], t["mask"], c.H, t["base"], out=o.views())
        assert out.data_ptr() == o.view("out").data_ptr()
        return o.collect(cid)

    def backward():
        o = Outputs(dev, MARGIN).with_results(dict(S=(c.B, c.taps, c.C)))
        L.cond_field_backward(t["dy"], t["mask"], c.taps, out=o.views())
        return o.collect(cid)

    got = dict(twice(forward, cid), **twice(backward, cid))
    fails = []
    for n in ("out", "S"):
        held(cid, n, got[n], ref[n], r32[n], fails)
        if c.ints:
            assert torch.equal(got[n].double(), ref[n]), (cid, n)
    assert not fails, (cid, fails)
    if not c.base:            # without a base the field is exactly zero wherever no tap reads a live column
        assert float((got["out"] * (ref["out"] == 0)).abs().max()) == 0.0, cid


@pytest.mark.parametrize("cid", [c.id for c in G.P_CASES])
def test_masked_mean_matches_float64(L, dev, cid):
    c, d, ref, r32 = refs("P", cid)
    t = guarded_inputs(d, ("y", "dp", "mask"), MARGIN, dev)

    def forward():
        o = Outputs(dev, MARGIN).with_results(dict(p=(c.B, c.C)))
        L.masked_mean(t["y"], t["mask"], out=o.views())
        return o.collect(cid)

    def backward():
        o = Outputs(dev, MARGIN).with_results(dict(dy=(c.B, c.C, c.H, c.W)))
        L.masked_mean_backward(t["dp"], t["mask"], c.H, out=o.views())
        return o.collect(cid)

    got = dict(twice(forward, cid), **twice(backward, cid))
    # RefBlock's tail with the pooling first: the 1x1 weight on the pooled vector, the bias unchanged
    got["tail"] = got["p"].double() @ d["wf"].double().view(G.P_COUT, c.C).t() + d["bf"].double()
    fails = []
    for n in ("p", "dy", "tail"):
        held(cid, n, got[n], ref[n], r32[n], fails)
    if c.ints:
        assert torch.equal(got["p"], ref["p"].float()) and torch.equal(got["dy"], ref["dy"].float()), cid
    assert not fails, (cid, fails)
    assert float((got["dy"] * (1.0 - d["mask"])[:, None, None, :]).abs().max()) == 0.0      # a masked column receives no gradient


@pytest.mark.parametrize("cid", [c.id for c in G.G_CASES])
def test_instance_norm_glu_with_time_bias_matches_float64(L, dev, cid):
    c, d, ref, r32 = refs("G", cid)
    t = guarded_inputs(d, ("y", "gamma", "beta", "tb", "dout"), MARGIN, dev)
    stats = {}

    def forward():
        o = Outputs(dev, MARGIN).with_results(dict(out=(c.B, c.C, c.H, c.W), stats=(int(L.lib().gtts_in_glu_stats_floats(c.B, c.C)),)))
        stats["s"] = L.in_glu_forward(t["y"], t["gamma"], t["beta"], G.G_EPS, tb=t["tb"], out=o.views())[1]
        return o.collect(cid)

    def backward():
        o = Outputs(dev, MARGIN).with_results(dict(dy=(c.B, 2 * c.C, c.H, c.W), dgamma=(2 * c.C,), dbeta=(2 * c.C,), dtb=(c.B, c.C)))
        L.in_glu_backward(t["dout"], t["y"], t["gamma"], t["beta"], stats["s"].clone(), want_dtb=True, out=o.views())
        return o.collect(cid)

    got = twice(forward, cid)
    _, plain_stats = L.in_glu_forward(t["y"], t["gamma"], t["beta"], G.G_EPS)
    assert torch.equal(plain_stats.cpu(), got["stats"]), cid                     # the statistics do not see the bias
    got.update(twice(backward, cid))
    fails = []
    for n in G.G_TENSORS:
        held(cid, n, got[n], ref[n], r32[n], fails)
    assert not fails, (cid, fails)
    # the bias changes nothing else: dy / dgamma / dbeta have the bits of the entry without it
    dy, dg, db = L.in_glu_backward(t["dout"], t["y"], t["gamma"], t["beta"], plain_stats)
    assert same_bits(dict(dy=dy.cpu(), dgamma=dg.cpu(), dbeta=db.cpu()), got), cid


@functools.lru_cache(maxsize=None)
def conv_refs(cid):
    c = G.N_BY_ID[cid]
    d = G.n_inputs(c)
    return c, d, G.n_composition(c, d), G.n_composition(c, d, torch.float32)


@pytest.mark.parametrize("cid", [c.id for c in G.N_CASES])
def test_narrow_convolution_matches_float64(L, dev, cid):
    """Forward, weight + bias gradient and (cin 32) data gradient of RefBlock's narrow layers: fp32 products and sums on the fp32-input
    MFMA, so they are held to the fp32 bound, not to the split-bf16 one of the wide layers."""
    c, d, ref, r32 = conv_refs(cid)
    t = guarded_inputs(d, ("x", "w", "bias", "dy", "mask"), MARGIN, dev)
    om = t["mask"] if c.omask else None
    ws = lambda op: int(L.lib().gtts_conv3x3_narrow_workspace_bytes(c.B, c.cin, c.cout, c.H, c.W, op)) // 4
    assert L.conv3x3_supported(c.cin, c.cout, need_dgrad=c.cin == 32, shape=(c.B, c.H, c.W)), cid

    def forward():
        o = Outputs(dev, MARGIN).with_results(dict(out=(c.B, c.cout, c.H, c.W)))
        L.conv3x3_narrow_forward(t["x"], t["mask"], t["w"], t["bias"], out_mask=om, out=dict(o.views(), workspace=o.space("workspace", ws(0))))
        return o.collect(cid)

    def wgrad():
        o = Outputs(dev, MARGIN).with_results(dict(dw=(c.cout, c.cin, 3, 3), db=(c.cout,)))
        L.conv3x3_narrow_wgrad(t["x"], t["mask"], t["dy"], out_mask=om, out=dict(o.views(), workspace=o.space("workspace", ws(2))))
        return o.collect(cid)

    def dgrad():
        o = Outputs(dev, MARGIN).with_results(dict(dx=(c.B, c.cin, c.H, c.W)))
        L.conv3x3_narrow_dgrad(t["dy"], t["w"], t["mask"], out_mask=om, out=dict(o.views(), workspace=o.space("workspace", ws(1))))
        return o.collect(cid)

    got = dict(y=twice(forward, cid)["out"], **twice(wgrad, cid))
    if c.cin == 32:
        got.update(twice(dgrad, cid))
    fails = []
    for n in got:
        held(cid, n, got[n], ref[n], r32[n], fails)
    assert not fails, (cid, fails)
    dead = (1.0 - d["mask"])[:, None, None, :]
    assert "dx" not in got or float((got["dx"] * dead).abs().max()) == 0.0                   # a masked column receives no gradient
    assert not c.omask or float((got["y"] * dead).abs().max()) == 0.0
    if not c.omask:           # what the module calls: the dispatch of conv3x3_masked / _dgrad / _wgrad gives the same bits
        y = L.conv3x3_masked(t["x"], t["mask"], t["w"], t["bias"]).cpu()
        dw, db = L.conv3x3_wgrad(t["x"], t["mask"], t["dy"])
        assert same_bits(dict(y=y, dw=dw.cpu(), db=db.cpu()), got), cid
        assert c.cin != 32 or same_bits(dict(dx=L.conv3x3_dgrad(t["dy"], t["w"], t["mask"]).cpu()), got), cid
