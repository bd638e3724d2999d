"""GPU parity tests (-m gpu) of the 2-D training convolutions of the decoder and of the DiffVC PostNet, one op at one shape through the
wrappers of _lib.py and through the autograd Functions of model/_train_ops.py, against torch autograd in float64 on the CPU.  The
catalogue is tests/dec_conv_train_cases.py (ops, value kinds, bounds); tests/test_dec_conv_train_cases_cpu.py proves without a GPU that
these bounds tell sixteen restated geometry mistakes and two arithmetic ones from the kernels' contract.

  bounds    `integers` cases: every element equal to the float64 reference.  Split-bf16 tensors: per element |got - ref| <= 2^-14 M, per
            tensor e = max |got - ref| / max |ref| <= 4 e_emul + 2e-6 and <= 1e-4.  fp32 tensors and every db: e <= 4 e_ref32 + 2e-6.
            The glue ops (zero_insert2, space_to_depth2, add_masked): the bits of the fp32 torch expression.  dx exactly 0 on masked frames.
  guards    x, dy, the masks, the bias and the weight before packing lie inside allocations whose margins hold NaN; every result and
            every workspace inside one filled with a sentinel: margins intact, every result element written, everything finite
  repeats   every call is made twice and gives the same bits
  instance  the kernel instance each forward / data-gradient call ran, from the dispatch that launched it (conv_train_kernel_name)
Run with -s for the table; the recorded figures are in profiles/dec_conv_train_parity.txt."""
import pytest
import torch

import dec_conv_train_cases as C
from gpu_guards import NAN, TO, L, Outputs, dev, guarded, guarded_inputs, table_row, twice  # noqa: F401

pytestmark = pytest.mark.gpu
MARGIN = 4096          # floats: above three rows of the widest case, a multiple of the 16-byte loads
CONV_IDS = [c.id for c in C.CASES if c.op in C.CONV_OPS]
GLUE_IDS = [c.id for c in C.CASES if c.op in C.GLUE_OPS]


def device_inputs(c, d, dev):
    """The case's inputs on the device, each inside NaN margins; a two-source input as its two tensors."""
    t = guarded_inputs(d, d, MARGIN, dev)
    if c.c0 and c.op == "c3":
        t["x"], t["x1"] = guarded(d["x"][:, :c.c0].contiguous(), MARGIN, NAN, dev)[0], guarded(d["x"][:, c.c0:].contiguous(), MARGIN, NAN, dev)[0]
    return t


def run_wrappers(L, c, t, dev):
    """{y, dx, dw, db} (those the op has) through the wrappers the autograd Functions call, every result and workspace between guards."""
    g = Outputs(dev, MARGIN)
    res = lambda name, *shape: g.result(name, shape)
    B, ci, co, H, W, k = c.B, c.cin, c.cout, c.H, c.W, c.k
    lib = L.lib()
    x, dy, w, bias, mask = t["x"], t["dy"], t["w"], t["bias"], t["mask"]
    wg = lambda floats: dict(dw=res("dw", *C.w_shape(c)), db=res("db", co) if C.has_bias(c) else None, workspace=g.space("ws", floats))
    if c.op in ("c3", "c1", "c7"):
        kind = C.REGIME_KIND[c.op]
        fwd, dgrad, wgrad = [getattr(L, "conv%s_%s" % (kind, f)) for f in ("masked", "dgrad", "wgrad")]
        extra = dict(x1=t.get("x1")) if c.op == "c3" else {}
        fwd(x, mask, w, bias, out=res("y", B, co, H, W), **extra)
        dgrad(dy, w, mask, out=res("dx", B, ci, H, W))
        nws = int(getattr(lib, "gtts_conv%s_wgrad_workspace_bytes" % kind)(B, ci, co, H, W)) // 4
        if c.op == "c1":
            wgrad(x, mask, dy, want_bias=C.has_bias(c), out=wg(nws))
        else:
            wgrad(x, mask, dy, out=wg(nws), **extra)
    elif c.op == "dn":
        L.conv_resample(x, mask, w, bias, False, out=res("y", B, co, H // 2, W // 2))
        gi = L.conv_resample(dy, L._const(dev, "ones", B, W // 2), w, None, True, dgrad_of_down=True, out=res("gi", B, ci, H, W))
        L.add_masked(None, gi, mask, out=res("dx", B, ci, H, W))
        z = L.zero_insert2(dy, out=res("z", B, co, H, W))
        L.conv3x3_wgrad(x, mask, z, out=wg(int(lib.gtts_conv3x3_wgrad_workspace_bytes(B, ci, co, H, W)) // 4))
    elif c.op == "up":
        L.conv_resample(x, mask, w, bias, True, out=res("y", B, co, 2 * H, 2 * W))
    elif c.op == "first":
        (L.conv3x3_masked if k == 3 else L.conv1x1_masked)(x, mask, w, bias, out=res("y", B, co, H, W))
        L.conv_dgrad_small(dy, w, mask, out=dict(dx=res("dx", B, ci, H, W)))
        (L.conv3x3_wgrad if k == 3 else L.conv1x1_wgrad)(x, mask, dy, out=wg(int(lib.gtts_conv_wgrad_small_scratch_floats(B, ci, co, k))))
    elif c.op == "final":
        L.final_conv_forward(x, w, bias, mask, out=res("y", B, 1, H, W))
        L.final_conv_backward(x, w, mask, dy, out=dict(dx=res("dx", B, ci, H, W), dw=res("dw", 1, ci, 1, 1), db=res("db", 1),
                                                         workspace=g.space("ws", int(lib.gtts_final_conv_scratch_floats(B, ci, H, W)))))
    elif c.op == "pexp":
        L.postnet_expand(x, mask, w, bias, out=res("y", B, co, H, W))
        L.postnet_collapse(dy, mask, w, out=res("dx", B, H, W))
        L.postnet_chan_dot(dy, x, mask, out=dict(dot=res("dw", co), sum=res("db", co),
                                                 workspace=g.space("ws", int(lib.gtts_postnet_chan_dot_scratch_floats(B, co, H, W)))))
    elif c.op == "pcol":
        L.postnet_collapse(x, mask, w, bias, out=res("y", B, H, W))
        L.postnet_expand(dy, mask, w, out=res("dx", B, ci, H, W))
        L.postnet_chan_dot(x, dy, mask, want_sum=False,
                           out=dict(dot=res("dw", ci), workspace=g.space("ws", int(lib.gtts_postnet_chan_dot_scratch_floats(B, ci, H, W)))))
        L.postnet_chan_dot(dy.unsqueeze(1), None, None, want_dot=False,
                           out=dict(sum=res("db", 1), workspace=g.space("ws1", int(lib.gtts_postnet_chan_dot_scratch_floats(B, 1, H, W)))))
    else:
        raise KeyError(c.op)
    return g.collect(c.id)


def check(c, got, ref, M, base, names, instances):
    """One table row per tensor, then the catalogue's bound of each."""
    bad = []
    for n in names:
        assert float(ref[n].abs().max()) > 0.0 and got[n].shape == ref[n].shape, (c.id, n, got[n].shape)
        e = C.relerr(got[n], ref[n])
        ratio = "%9.2e" % C.worst_ratio(got[n], ref[n], M[n]) if C.split_bf16(c, n) else "        -"
        table_row(__name__, "\n%-46s %-3s %-66s %10s %9s %9s %9s" % ("case", "", "kernel instance", "max|ref|", "e", "e_base", "|err|/M"),
                  "%-46s %-3s %-66s %10.3e %9.2e %9.2e %s" % (c.id, n, instances.get(n, "-"), float(ref[n].abs().max()), e, base[n], ratio))
        if not C.passes(c, n, got[n], ref[n], M[n], base[n]):
            bad.append((n, e, base[n], ratio))
    assert not bad, (c.id, bad)


def masked_frames_are_zero(c, dx):
    if C.has_mask(c):
        for b, n in enumerate(c.lens):
            assert n == c.W or float(dx[b, ..., n:].abs().max()) == 0.0, (c.id, b)


@pytest.mark.parametrize("cid", CONV_IDS)
def test_wrappers_match_float64(L, dev, cid):
    c, d, ref, M, base = C.references(cid)
    t = device_inputs(c, d, dev)
    got = twice(lambda: run_wrappers(L, c, t, dev))
    check(c, got, ref, M, base, C.tensor_names(c), C.instances(c, L.conv_train_kernel_name))
    if "dx" in got:
        masked_frames_are_zero(c, got["dx"])
    if c.op == "dn":          # the pieces on the way: the zero-inserted dy is dy at the even positions and exact zeros elsewhere
        assert torch.equal(got["z"], C._zero_insert(d["dy"])), cid


@pytest.mark.parametrize("cid", GLUE_IDS)
def test_glue_ops_have_the_bits_of_the_torch_expression(L, dev, cid):
    c = C.BY_ID[cid]
    d = C.make_inputs(c)
    ref = C.glue_reference(c, d)
    t = device_inputs(c, d, dev)

    def run():
        g = Outputs(dev, MARGIN)
        out = g.result("out", ref.shape)
        if c.op == "zi":
            L.zero_insert2(t["b"], out=out)
        elif c.op == "s2d":
            L.space_to_depth2(t["b"], out=out)
        elif c.op == "am":
            L.add_masked(t["a"], t["b"], t["mask"], out=out)
        else:
            L.add_masked(None, t["b"], t["mask"], channels=(c.c0, c.c0 + c.cout), out=out)
        return g.collect(cid)

    got = twice(run)
    assert torch.equal(got["out"], ref), cid


def _mask4(t):
    return None if t["mask"] is None else t["mask"][:, None, None, :]


def apply_function(TO, c, t, x, x1, w, b):
    """The op's autograd Function on leaves x (x1), w, b."""
    if c.op in ("c3", "first") and c.k == 3:
        return TO.MaskedConv3x3.apply(x, _mask4(t), w, b, x1)
    if c.op in ("c1", "first"):
        return TO.MaskedConv1x1.apply(x, _mask4(t), w, b)
    if c.op == "c7":
        return TO.MaskedConv7x7.apply(x, _mask4(t), w, b)
    if c.op in ("dn", "up"):
        return TO.ResampleConv.apply(x, _mask4(t), w, b, c.op == "up")
    if c.op == "final":
        return TO.FinalConv.apply(x, _mask4(t), w, b)
    return (TO.PostNetInitConv if c.op == "pexp" else TO.PostNetFinalConv).apply(x, t["mask"], w, b)


def gate(L, c):
    """What model/_train_ops.py asks before it takes the kernels: a refusal there is a silent torch fallback in a training step."""
    shape = (c.B, c.H, c.W)
    if c.op in ("c3", "first") and c.k == 3:
        return L.conv3x3_supported(c.cin, c.cout, shape=shape)
    if c.op in ("c1", "first"):
        return L.conv1x1_supported(c.cin, c.cout, shape=shape)
    if c.op == "c7":
        return L.conv7x7_supported(c.cin, c.cout, shape=shape)
    if c.op in ("dn", "up"):
        return L.resample_supported(c.cin, c.cout, c.H, c.W, c.op == "up", B=c.B)
    return True


@pytest.mark.parametrize("cid", CONV_IDS)
def test_autograd_functions_match_the_wrappers(L, TO, dev, cid):
    """MaskedConv3x3 (one and two sources, first layer), MaskedConv1x1, MaskedConv7x7, ResampleConv, FinalConv, PostNetInitConv and
    PostNetFinalConv on the same cases: forward and gradients have the bits of the wrapper calls (Upsample's gradients, which exist only
    inside ResampleConv.backward, are held to the catalogue's bounds against float64), an input that needs no gradient gets None, the
    gates of the training path accept the shape and nothing is counted as a fallback."""
    c, d, ref, M, base = C.references(cid)
    assert gate(L, c), cid
    t = device_inputs(c, d, dev)
    want = run_wrappers(L, c, t, dev)
    TO.reset_op_counts()
    leaf = lambda v, need=True: None if v is None else v.clone().requires_grad_(need)
    x, x1, w, b = leaf(t["x"]), leaf(t.get("x1")), leaf(t["w"]), leaf(t["bias"])
    if c.op in ("dn", "up") or c.op == "final" or c.op in ("pexp", "pcol"):
        assert b is not None
    y = apply_function(TO, c, t, x, x1, w, b)
    y.backward(t["dy"])
    torch.cuda.synchronize()
    assert torch.equal(y.detach().cpu(), want["y"]), cid
    dx = x.grad if x1 is None else torch.cat((x.grad, x1.grad), 1)
    got = dict(y=y.detach().cpu(), dx=dx.cpu(), dw=w.grad.cpu(), db=None if b is None else b.grad.cpu())
    if c.op == "up":
        check(c, got, ref, M, base, ["dx", "dw", "db"], {})
    else:
        for n in ("dx", "dw", "db"):
            assert got[n] is None or torch.equal(got[n], want[n]), (cid, n)
    masked_frames_are_zero(c, got["dx"])
    # an input that needs no gradient gets none, and the weight gradient keeps its bits
    x2, x12, w2, b2 = leaf(t["x"], False), leaf(t.get("x1"), False), leaf(t["w"]), leaf(t["bias"], False)
    y2 = apply_function(TO, c, t, x2, x12, w2, b2)
    y2.backward(t["dy"])
    assert x2.grad is None and (x12 is None or x12.grad is None) and (b2 is None or b2.grad is None)
    assert torch.equal(w2.grad, w.grad), cid
    assert TO.op_counts()[1] == 0


def test_out_arguments_are_checked(L, dev):
    """A preallocated result or workspace of the wrong shape, dtype or device, or a non-contiguous one, is refused before any launch."""
    c = C.BY_ID["c3-plain-b2-64to64-3x7"]
    d = {k: (None if v is None else v.to(dev)) for k, v in C.make_inputs(c).items()}
    x, dy, w, bias, mask = d["x"], d["dy"], d["w"], d["bias"], d["mask"]
    good = torch.empty(2, 64, 3, 7, device=dev)
    bad = (torch.empty(2, 64, 3, 8, device=dev), torch.empty(2, 64, 3, 7, device=dev, dtype=torch.float64), torch.empty(2, 64, 3, 7),
           torch.empty(2, 64, 7, 3, device=dev).transpose(2, 3))
    for out in bad:
        for call in (lambda o: L.conv3x3_masked(x, mask, w, bias, out=o), lambda o: L.conv3x3_dgrad(dy, w, mask, out=o),
                     lambda o: L.conv7x7_dgrad(dy, torch.zeros(64, 64, 7, 7, device=dev), mask, out=o),
                     lambda o: L.conv1x1_masked(x, mask, torch.zeros(64, 64, 1, 1, device=dev), None, out=o),
                     lambda o: L.add_masked(None, x, mask, out=o), lambda o: L.postnet_expand(x[:, 0], mask, w[:, 0, 0, 0], out=o),
                     lambda o: L.conv_resample(torch.zeros(2, 64, 6, 14, device=dev), torch.ones(2, 14, device=dev), w, bias, False, out=o)):
            with pytest.raises(ValueError):
                call(out)
    nws = int(L.lib().gtts_conv3x3_wgrad_workspace_bytes(2, 64, 64, 3, 7)) // 4
    ok = dict(dw=torch.empty(64, 64, 3, 3, device=dev), db=torch.empty(64, device=dev), workspace=torch.empty(nws, device=dev))
    for name, wrong in (("dw", torch.empty(64, 64, 9, device=dev)), ("db", torch.empty(64, device=dev, dtype=torch.float16)),
                        ("workspace", torch.empty(nws - 1, device=dev)), ("workspace", torch.empty(nws, dtype=torch.float32))):
        with pytest.raises(ValueError):
            L.conv3x3_wgrad(x, mask, dy, out=dict(ok, **{name: wrong}))
    with pytest.raises(ValueError):
        L.final_conv_backward(x, torch.zeros(1, 64, 1, 1, device=dev), mask, dy[:, :1], out=dict(dx=good[:, :32]))
    with pytest.raises(ValueError):
        L.postnet_chan_dot(x, None, None, out=dict(dot=torch.empty(63, device=dev)))
    # and what is right is used: the result comes back in the caller's tensor
    assert L.conv3x3_masked(x, mask, w, bias, out=good).data_ptr() == good.data_ptr()
    dw, db = L.conv3x3_wgrad(x, mask, dy, out=ok)
    assert dw.data_ptr() == ok["dw"].data_ptr() and db.data_ptr() == ok["db"].data_ptr()
