"""GPU parity tests (-m gpu) of the shared 1-D convolution kernel (csrc/conv1d.h), one layer at one shape through Conv1dOp -- the
single-layer entry to the launcher that the vocoder and both encoders use -- against torch's conv1d / conv_transpose1d in float64 on the
CPU.  The catalogue is tests/conv1d_cases.py; tests/test_conv1d_cases_cpu.py proves it selects all nine instances and every epilogue.

  reference   leaky_relu(x, slope) * in_mask -> conv -> + bias, + res, running sum, division, * out_mask, in float64
  error       e = max |got - ref| / max |ref| over ALL elements; bound REL = 1e-4 (split-bf16 contractions)
  e32         the same op in float32 torch against float64: the float32 reference's own error, printed beside e
  guards      x, res, accsrc, the masks and the bias lie inside larger allocations whose margins (>= 16 * Lin * S floats each side:
              farther than any read the staging can issue, pad channels included) hold NaN, `out` inside one filled with a sentinel:
              the result must be finite, every element of `out` written, the margins untouched
Run with -s for the table; the recorded figures are in profiles/conv1d_parity.txt."""
import pytest
import torch

import conv1d_cases as C
from gpu_guards import SENTINEL, Outputs, S, dev, guarded_inputs, table_row  # noqa: F401

pytestmark = pytest.mark.gpu


def run_case(S, dev, c, d, op=None):
    """The layer on the GPU between guards; returns the CPU result after checking the margins of `out`."""
    op = op or S.Conv1dOp(**C.op_kwargs(c))
    margin = 16 * c.Lin * c.S + 64
    t = guarded_inputs(d, ("x", "bias", "res", "accsrc", "in_mask", "out_mask"), margin, dev)
    o = Outputs(dev, margin)
    out = o.result("out", (c.B, c.cout, c.Lin * c.S))
    blob = op.pack(d["w"], dev)
    got = op.forward(blob, t["bias"], t["x"], out=out, res=t["res"], accsrc=t["accsrc"], accmode=c.accmode, div=c.div, slope=c.slope,
                     in_mask=t["in_mask"], out_mask=t["out_mask"])
    assert got.data_ptr() == out.data_ptr()
    return o.collect(c.id, values=False)["out"]          # written / finite: asserted by the caller, after its table row


@pytest.mark.parametrize("cid", [c.id for c in C.CASES])
def test_layer_matches_float64(S, dev, cid):
    c = C.BY_ID[cid]
    d = C.make_inputs(c)
    ref = C.reference(c, d)
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0.1
    e32 = C.relerr(C.reference(c, d, torch.float32), ref)
    op = S.Conv1dOp(**C.op_kwargs(c))
    inst = op.instance(c.B, c.Lin, res=c.res, accmode=c.accmode, out_mask=c.out_lens is not None)
    got = run_case(S, dev, c, d, op)
    finite = bool(torch.isfinite(got).all())
    e = C.relerr(got, ref) if finite else float("nan")
    table_row(__name__, "\n%-28s %-22s %-8s %9s %9s %9s" % ("case", "instance MT,TPS,AI,KCH", "epilogue", "max|ref|", "e", "e32"),
              "%-28s %-22s %-8s %9.3f %9.2e %9.2e" % (c.id, "%d,%d,%d,%d" % inst[:4], C.EPI_NAME[inst[4]], float(ref.abs().max()), e, e32))
    assert finite, "%s: non-finite output (a read outside the input reached the result)" % c.id
    assert not bool((got == SENTINEL).any()), "%s: an output element was never written" % c.id
    assert e <= C.REL, (c.id, e)
    if c.out_lens is not None:
        # beyond an utterance's length the output is exactly 0, whatever bias, residual and running sum hold there
        for b, n in enumerate(c.out_lens):
            assert n == got.shape[-1] or float(got[b, :, n:].abs().max()) == 0.0, (c.id, b)
            assert n == 0 or float(got[b, :, :n].abs().max()) > 0.0, (c.id, b)


def test_kch2_is_bit_identical_to_kch1(S, dev):
    """The KCH = 2 instance (32 channels per step) issues its MFMAs in the order of two consecutive 16-channel steps: a k = 3,
    32 -> 128 channel layer (KCH = 2) and the same layer with 16 zero input channels and zero weights appended (48 channels, an odd
    number of chunks: KCH = 1) must agree bit for bit -- the extra chunk adds exact zeros to every accumulator."""
    c = C.case("kch2-vs-kch1", 32, 128, 3, 200, B=2, slope=0.1)
    c48 = c._replace(cin=48)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(c.B, 32, c.Lin, generator=g)
    w = (torch.rand(128, 32, 3, generator=g) * 2 - 1) / 96 ** 0.5
    bias = torch.rand(128, generator=g) - 0.5
    d = dict(x=x, w=w, bias=bias, res=None, accsrc=None, in_mask=None, out_mask=None)
    d48 = dict(d, x=torch.cat([x, torch.zeros(c.B, 16, c.Lin)], 1).contiguous(), w=torch.cat([w, torch.zeros(128, 16, 3)], 1).contiguous())
    op, op48 = S.Conv1dOp(**C.op_kwargs(c)), S.Conv1dOp(**C.op_kwargs(c48))
    assert op.instance(c.B, c.Lin)[:4] == (128, 3, 3, 2) and op48.instance(c.B, c.Lin)[:4] == (128, 3, 2, 1)
    a, b = run_case(S, dev, c, d, op), run_case(S, dev, c48, d48, op48)
    assert C.relerr(a, C.reference(c, d)) <= C.REL
    assert torch.equal(a, b), "KCH = 2 differs from KCH = 1: max |diff| %.3e" % float((a - b).abs().max())


def test_output_may_be_given_or_allocated(S, dev):
    """forward() without `out` allocates it; the same bits as the guarded call."""
    c = C.BY_ID["epi-whole-acc2"]
    d = C.make_inputs(c)
    op = S.Conv1dOp(**C.op_kwargs(c))
    a = run_case(S, dev, c, d, op)
    b = op.forward(op.pack(d["w"], dev), d["bias"].to(dev), d["x"].to(dev), res=d["res"].to(dev), accsrc=d["accsrc"].to(dev),
                   accmode=c.accmode, div=c.div, slope=c.slope).cpu()
    assert torch.equal(a, b)
