"""GPU parity tests (-m gpu) of the encoders' Conv1d training path, one layer at one shape through the binding (Conv1dOp.pack_into /
forward / pack_dgrad / wgrad) and through the autograd Function (EncConv1d), against torch autograd in float64 on the CPU.  The catalogue is
tests/enc_conv_train_cases.py; tests/test_enc_conv_train_cases_cpu.py proves which regimes of the weight-gradient launcher it reaches.

  error    e = max |got - ref| / max |ref| per tensor over ALL elements, bound 1e-4 (split-bf16 contractions, fp32 accumulate); db, a
           plain fp32 sum, additionally e <= 4 e_ref32 + 2e-6 with e_ref32 the same autograd in fp32 torch on the CPU
  guards   x, dy, the masks and the zero bias lie inside larger allocations whose margins hold NaN; dx, dw, db and the workspace inside
           ones filled with a sentinel: results finite, every element written, the margins intact
  bits     two backward calls agree bit for bit; pack_dgrad equals the ordinary pack of the flipped, transposed weight; EncConv1d's
           forward equals Conv1dOp.forward
Run with -s for the table; the recorded figures are in profiles/enc_conv_train_parity.txt."""
import pytest
import torch

import enc_conv_train_cases as C
from gpu_guards import NAN, TO, Outputs, S, dev, guarded, guarded_inputs, table_row  # noqa: F401

pytestmark = pytest.mark.gpu


def backward_through_binding(S, dev, c, d):
    """dx (None when the case asks for none), dw, db (None without a bias) on the GPU between guards."""
    fwd, tr = S.Conv1dOp(0, c.cin, c.cout, c.K, c.dil), S.Conv1dOp(0, c.cout, c.cin, c.K, c.dil)
    margin = 16 * c.L * (c.K * c.dil + 1) + 64
    t = guarded_inputs(d, ("x", "dy", "in_mask", "out_mask", "w"), margin, dev)
    zero = guarded(torch.zeros(c.cin), margin, NAN, dev)[0]
    o = Outputs(dev, margin)
    if c.x_grad:
        tr.forward(tr.pack_dgrad(t["w"]), zero, t["dy"], out=o.result("dx", (c.B, c.cin, c.L)), in_mask=t["out_mask"], out_mask=t["in_mask"])
    nws = fwd.wgrad_workspace_bytes(c.B, c.L)
    assert nws % 4 == 0
    fwd.wgrad(t["x"], t["dy"], t["in_mask"], t["out_mask"], want_bias=c.bias, dw=o.result("dw", (c.cout, c.cin, c.K)),
              db=o.result("db", (c.cout,)) if c.bias else None, workspace=o.space("workspace", nws // 4))
    got = o.collect(c.id)
    return got.get("dx"), got["dw"], got.get("db")


@pytest.mark.parametrize("cid", [c.id for c in C.CASES])
def test_gradients_match_float64(S, dev, cid):
    c = C.BY_ID[cid]
    d = C.make_inputs(c)
    ref, ref32 = C.reference(c, d), C.reference(c, d, torch.float32)
    dx, dw, db = backward_through_binding(S, dev, c, d)
    dx2, dw2, db2 = backward_through_binding(S, dev, c, d)
    rows = [("dw", dw, ref["dw"], ref32["dw"])]
    if c.x_grad:
        rows.append(("dx", dx, ref["dx"], ref32["dx"]))
    if c.bias:
        rows.append(("db", db, ref["db"], ref32["db"]))
    info = S.Conv1dOp(0, c.cin, c.cout, c.K, c.dil).wgrad_info(c.B, c.L)
    bad = []
    for name, got, r64, r32 in rows:
        assert float(r64.abs().max()) > 0.0
        e, e32 = C.relerr(got, r64), C.relerr(r32, r64)
        table_row(__name__, "\n%-20s %-22s %-4s %9s %9s %9s" % ("case", "slices,per,empty", "", "max|ref|", "e", "e_ref32"),
                  "%-20s %-22s %-4s %9.3f %9.2e %9.2e" % (c.id, "%d,%d,%d" % info[3:], name, float(r64.abs().max()), e, e32))
        if not e <= C.REL or (name == "db" and not e <= C.db_bound(e32)):
            bad.append((name, e, e32))
    assert not bad, (c.id, bad)
    # two calls, the same bits
    assert torch.equal(dw, dw2) and (db is None or torch.equal(db, db2)) and (dx is None or torch.equal(dx, dx2)), c.id
    # beyond an utterance's input length the input gradient is exactly 0
    if c.x_grad and c.in_lens is not None:
        for b, n in enumerate(c.in_lens):
            assert n == c.L or float(dx[b, :, n:].abs().max()) == 0.0, (c.id, b)


@pytest.mark.parametrize("cid", ["module-24-48-k3", "ffn-192-768-k3", "proj-192-80-k1", "dp-256-1-k1", "dil3-k5", "slice-empty"])
def test_pack_dgrad_equals_the_pack_of_the_flipped_transposed_weight(S, dev, cid):
    c = C.BY_ID[cid]
    w = C.make_inputs(c)["w"].to(dev)
    tr = S.Conv1dOp(0, c.cout, c.cin, c.K, c.dil)
    a = tr.pack_dgrad(w)
    b = tr.pack(w.transpose(0, 1).flip(-1).contiguous(), dev)
    also = tr.pack_into(w.transpose(0, 1).flip(-1).contiguous())
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(also, b)


@pytest.mark.parametrize("cid", [c.id for c in C.CASES])
def test_autograd_function_matches_the_binding_and_float64(S, TO, dev, cid):
    """EncConv1d: its forward has the bits of Conv1dOp.forward (kernel_forward) or the fp32 grade of torch's conv1d on the device (the
    form the encoders are wired with: e <= 4 e_ref32 + 2e-6), its gradients those of the binding calls either way; a case whose input needs no gradient gets none, a case
    without a bias no bias gradient."""
    c = C.BY_ID[cid]
    d = C.make_inputs(c)
    ref = C.reference(c, d)
    mv = lambda v: None if v is None else v.to(dev)
    x = mv(d["x"]).requires_grad_(c.x_grad)
    w = mv(d["w"]).requires_grad_(True)
    b = None if d["bias"] is None else mv(d["bias"]).requires_grad_(True)
    im, om = mv(d["in_mask"]), mv(d["out_mask"])
    y = TO.EncConv1d.apply(x, w, b, im, om, c.dil, True)
    y.backward(mv(d["dy"]))
    op = S.Conv1dOp(0, c.cin, c.cout, c.K, c.dil)
    bias = torch.zeros(c.cout, device=dev) if b is None else b.detach()
    y_op = op.forward(op.pack(d["w"], dev), bias, x.detach(), in_mask=im, out_mask=om)
    assert torch.equal(y.detach(), y_op)
    assert C.relerr(y.detach().cpu(), ref["y"]) <= C.REL
    dx, dw, db = backward_through_binding(S, dev, c, d)
    assert torch.equal(w.grad.cpu(), dw)
    assert (x.grad is None) == (not c.x_grad) and (not c.x_grad or torch.equal(x.grad.cpu(), dx))
    assert b is None or torch.equal(b.grad.cpu(), db)
    # ... and with torch's forward: the module call's bits forward, the same kernels backward
    first = (w.grad.clone(), None if x.grad is None else x.grad.clone(), None if b is None else b.grad.clone())
    x.grad = w.grad = None
    if b is not None:
        b.grad = None
    y_t = TO.EncConv1d.apply(x, w, b, im, om, c.dil, False)
    y_t.backward(mv(d["dy"]))
    # (torch's convolution picks its algorithm per call, so two calls need not agree bit for bit: the forward is held to the fp32 grade)
    e32 = C.relerr(C.reference(c, d, torch.float32)["y"], ref["y"])
    assert C.relerr(y_t.detach().cpu(), ref["y"]) <= C.db_bound(e32), (cid, C.relerr(y_t.detach().cpu(), ref["y"]), e32)
    assert torch.equal(w.grad, first[0]) and (first[1] is None or torch.equal(x.grad, first[1])) and (b is None or torch.equal(b.grad, first[2]))
