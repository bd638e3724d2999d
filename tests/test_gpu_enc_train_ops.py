"""GPU parity tests (-m gpu) of the encoders' training kernels (csrc/enc_train.hip), one op at a time through
gtts_enc_attention_train_forward / _backward and gtts_enc_layernorm_backward against float64 autograd on the CPU.  The catalogue is
tests/enc_train_op_cases.py; tests/test_enc_train_op_cases_cpu.py proves its caps, its restatements and that the bound below tells
restated backward mistakes from the kernels.

  error     per gradient tensor  e = max |got - ref64| / max |ref64|  over ALL elements (padded queries and keys, the fully masked item
            and the length-1 item included); e_ref32 = the same autograd in fp32 torch on the CPU
  bound     e <= 4 e_ref32 + 2e-6 and e <= 1e-4; dq, dk, dek of the saturated regime: finite only.  The training forward without a
            multiplier is held to the forward bound of tests/enc_op_cases.py (e <= 4 e_ref32 + 2e-6 and e <= 1e-5)
  guards    every input lies inside a larger allocation whose margins hold NaN, every output inside one filled with a sentinel
  repeats   a second backward on the same inputs is torch.equal to the first, tensor by tensor
Run with -s for the table."""
import functools

import pytest
import torch

import enc_op_cases as K
import enc_train_op_cases as T
from gpu_guards import NAN, SENTINEL, Outputs, S, dev, guarded_inputs, table_row, twice  # noqa: F401

pytestmark = pytest.mark.gpu


def run_att(S, dev, c, d, drop=None):
    """Forward + backward of one case through the ABI wrappers -> dict(out, stat, dq, dk, dv[, dek, dev]); the backward runs again
    into fresh outputs and must give the same bits.  Only the margins are checked here: written / finite are asserted by the tests,
    after their table row."""
    B, C, L, H, w = c.B, c.heads * c.dk, c.L, c.heads, c.window
    margin = 4 * L + 256
    t = guarded_inputs(dict(d, dout=T.att_dout(c), drop=drop), ("q", "k", "v", "mask", "ek", "ev", "dout", "drop"), margin, dev)
    fshapes = dict(out=(B, C, L), stat=(B, H, L, 2))
    gshapes = dict(dq=(B, C, L), dk=(B, C, L), dv=(B, C, L))
    if w:
        gshapes.update(dek=(2 * w + 1, c.dk), dev=(2 * w + 1, c.dk))
    fo = Outputs(dev, margin).with_results(fshapes)
    out, stat = S.enc_attention_train_forward(t["q"], t["k"], t["v"], t["mask"], t["ek"], t["ev"], t["drop"], n_heads=H, window=w,
                                              out=fo.view("out"), stat=fo.view("stat"))
    assert out.data_ptr() == fo.view("out").data_ptr()
    got = fo.collect(values=False)

    def backward():
        go = Outputs(dev, margin).with_results(gshapes)
        S.enc_attention_train_backward(t["q"], t["k"], t["v"], t["mask"], t["ek"], t["ev"], t["drop"], stat, t["dout"], n_heads=H, window=w,
                                       grads=go.views())
        return go.collect(values=False)

    got.update(twice(backward, c.id))
    return got


@functools.lru_cache(maxsize=None)
def att_ref(cid, dropped):
    """(case, inputs, multiplier, float64 gradients, fp32 gradients): computed once per process, never modified."""
    c = T.ATT_TRAIN_BY_ID[cid]
    d = T.att_train_inputs(c)
    drop = T.att_drop(c) if dropped else None
    return c, d, drop, T.att_grads(c, d, drop=drop), T.att_grads(c, d, torch.float32, drop=drop)


def _row(kind, cid, name, maxref, e, e32, b, note=""):
    table_row((__name__, kind), "\n%-46s %-7s %10s %9s %9s %9s" % ("case", "tensor", "max|ref|", "e", "e_ref32", "bound"),
              "%-46s %-7s %10.3e %9.2e %9.2e %9.2e %s" % (cid, name, maxref, e, e32, b, note))


def _check_att(cid, dropped, S, dev):
    c, d, drop, ref, r32 = att_ref(cid, dropped)
    got = run_att(S, dev, c, d, drop)
    fails = []
    # ---- the forward
    e32 = K.relerr(r32["out"], ref["out"])
    e = K.relerr(got["out"], ref["out"]) if bool(torch.isfinite(got["out"]).all()) else NAN
    _row("att", cid, "out", float(ref["out"].abs().max()), e, e32, K.bound(e32), "drop" if dropped else "")
    assert not bool((got["out"] == SENTINEL).any()) and not bool((got["stat"] == SENTINEL).any()), "%s: an element was never written" % cid
    assert bool(torch.isfinite(got["stat"]).all())
    if not (e <= 4.0 * e32 + K.ELEMENTWISE_ABS and e <= K.REDUCTION_REL):
        fails.append(("out", e, e32))
    # ---- the five gradients
    for n in T.ATT_GRADS:
        if ref[n] is None:
            assert n not in got
            continue
        g = got[n]
        assert not bool((g == SENTINEL).any()), "%s: an element of %s was never written" % (cid, n)
        finite = bool(torch.isfinite(g).all())
        assert finite, "%s: non-finite %s" % (cid, n)
        e32, e = T.relerr(r32[n], ref[n]), T.relerr(g, ref[n])
        hold = T.held(c, n)
        _row("att", cid, n, float(ref[n].abs().max()), e, e32, T.bound(e32), "" if hold else "finite only")
        if hold:
            assert e32 <= T.E32_CAP[c.regime], (cid, n, e32)
            if not (e <= 4.0 * e32 + T.GRAD_ABS and e <= T.GRAD_REL):
                fails.append((n, e, e32))
    assert not fails, (cid, fails)


@pytest.mark.parametrize("cid", [c.id for c in T.ATT_TRAIN_CASES])
def test_attention_training_matches_float64(S, dev, cid):
    _check_att(cid, False, S, dev)


@pytest.mark.parametrize("cid", T.DROP_IDS)
def test_attention_training_with_a_dropout_multiplier_matches_float64(S, dev, cid):
    _check_att(cid, True, S, dev)


def test_forward_without_a_multiplier_agrees_with_the_inference_kernels(S, dev):
    """Same formulas, another association of the long sums: both within the forward bound, and within twice the bound of each other."""
    n = 0
    for c in K.ATT_SMALL[::5]:
        _, d, _, ref, r32 = att_ref(c.id, False)
        b = K.bound(K.relerr(r32["out"], ref["out"]))
        t = {k: (None if d[k] is None else d[k].to(dev)) for k in ("q", "k", "v", "mask", "ek", "ev")}
        inf = S.enc_attention(t["q"], t["k"], t["v"], t["mask"], t["ek"], t["ev"], n_heads=c.heads, window=c.window).cpu()
        trn = S.enc_attention_train_forward(t["q"], t["k"], t["v"], t["mask"], t["ek"], t["ev"], None, n_heads=c.heads, window=c.window)[0].cpu()
        diff = float((inf.double() - trn.double()).abs().max() / ref["out"].abs().max())
        assert diff <= 2.0 * b, (c.id, diff, b)
        n += 1
    assert n >= 10


# ------------------------------------------------------------------------------------------------------------------- LayerNorm
@functools.lru_cache(maxsize=None)
def ln_ref(cid):
    c = K.LN_BY_ID[cid]
    d = K.ln_inputs(c)
    return c, d, T.ln_grads(c, d), T.ln_grads(c, d, torch.float32)


def run_ln(S, dev, c, d):
    B, C, L = c.B, c.C, c.L
    margin = 16 * L + 256
    t = guarded_inputs(dict(d, dout=T.ln_dout(c)), ("dout", "a", "bres", "gamma", "beta", "a_mask", "out_mask"), margin, dev)
    shapes = dict(da=(B, C, L), dgamma=(C,), dbeta=(C,))
    if c.bres:
        shapes["dbres"] = (B, C, L)

    def backward():
        go = Outputs(dev, margin).with_results(shapes)
        S.enc_layernorm_backward(t["dout"], t["a"], t["gamma"], t["beta"], bres=t["bres"], a_mask=t["a_mask"], out_mask=t["out_mask"],
                                 eps=K.EPS, relu_in=c.relu_in, relu_out=c.relu_out, grads=go.views())
        return go.collect(values=False)

    return twice(backward, c.id)


@pytest.mark.parametrize("cid", [c.id for c in K.LN_CASES])
def test_layernorm_backward_matches_float64(S, dev, cid):
    c, d, ref, r32 = ln_ref(cid)
    got = run_ln(S, dev, c, d)
    fails = []
    for n in T.LN_GRADS:
        if ref[n] is None:
            assert n not in got
            continue
        g = got[n]
        assert not bool((g == SENTINEL).any()), "%s: an element of %s was never written" % (cid, n)
        assert bool(torch.isfinite(g).all()), "%s: non-finite %s (a read outside an input)" % (cid, n)
        e32, e = T.relerr(r32[n], ref[n]), T.relerr(g, ref[n])
        _row("ln", cid, n, float(ref[n].abs().max()), e, e32, T.bound(e32), c.data)
        assert e32 <= (T.LN_E32_CAP_OFFSET_DGAMMA if (c.data == "offset" and n == "dgamma") else T.LN_E32_CAP), (cid, n, e32)
        if not (e <= 4.0 * e32 + T.GRAD_ABS and e <= T.GRAD_REL):
            fails.append((n, e, e32))
    assert not fails, (cid, fails)
    if c.a_mask:                                              # a masked input column receives no gradient
        for b, n in enumerate(c.lens):
            assert n == c.L or float(got["da"][b, :, n:].abs().max()) == 0.0, (cid, b)
