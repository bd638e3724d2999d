"""GPU tests (-m gpu) of the level-0 attention output folded into the Downsample weights (csrc/attn.hip attn_fold, conv_mfma.hip
EPI_DNFOLD, plan.hip): the apply pass of downs.0.2 is not run, downs.0.3 reads the attention's INPUT with per-sample weights.

State: Rezero.g = 1.0 -- the attention branch and its bias at full strength (with the fixtures' g = 0.02 a wrong border term
would be 50x smaller).  Shape: B = 3, T = 72, lengths [72, 41, 1]: a tile edge inside the width (36 output columns, 32-column
tiles), an odd-length and a one-frame utterance.

Tolerance: REL = 1e-4 of tests/test_gpu_parity_full.py (bf16x3 contractions with fp32 accumulation).

Measured on MI355X (profiles/r08_fold_down_error.txt), max |err| / max |ref| of downs.0.3.out against F.conv2d on the HIP path's
own downs.0.2.out, worst region: folded 6.4e-6 (conv_mfma) / 5.9e-6 (f16f8 on conv_ws); the unfused path before the fold, same
inputs: 7.9e-6 / 4.8e-6.  Against the oracle's tap: at most 3.3e-5.

With g = 1.0 at all six attentions this state grows to 4.5e9 at the input of ups.1.2 in the ONE-FRAME utterance (branch 4.4e18) and
stays inside fp32 (CPU oracle: final output max 7.9).  bf16x3: the estimator output of all three utterances is finite on the HIP
path, since the context kernels take the softmax reference point exactly (tests/test_gpu_attention.py, profiles/attention_parity.txt).
f16f8: a range limit of the format (tests/test_gpu_range.py, contract (b)).  The split's hi operand is fp16, and in the one-frame
utterance the input of the 3x3 convolution of mid_block2.block1 (mid_attn.out, 1.5e6) is the first beyond 65504 -- the first
non-finite tap of the f16f8 plan is mid_block2.b1.raw, on both convolution kernels (walk: profiles/attention_parity.txt) -- and the up path then reaches 4.4e18.  That utterance is not finite there, utterances 0 and 1 are, and Plan.range_status() must report the limit:
events > 0 and max |x| = inf (non-finite GroupNorm statistics).  Both tests assert this per precision."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from oracle import diffvc_oracle as V
from oracle import gradtts_oracle as O
from gpu_guards import S, dev  # noqa: F401

pytestmark = pytest.mark.gpu
REL = 1e-4
B, T, LENGTHS = 3, 72, [72, 41, 1]

precs = pytest.mark.parametrize("prec", ["bf16x3", "f16f8"])
kernels = pytest.mark.parametrize("conv_ws", [False, True], ids=["conv_mfma", "conv_ws"])


@pytest.fixture(scope="module")
def case():
    """State, inputs and the CPU oracle's taps: computed once, shared, never modified."""
    sd = O.make_estimator_state(seed=5, rezero_g=1.0)
    inp = O.make_inputs(B, T, seed=99)
    lengths = torch.tensor(LENGTHS)
    mask = O.sequence_mask(lengths, T).unsqueeze(1).float()
    t = torch.linspace(0.15, 0.9, B)
    taps = {}
    ref = O.estimator_forward(sd, inp["z"], mask, inp["mu"], t, taps=taps)
    return {"sd": sd, "z": inp["z"], "mu": inp["mu"], "mask": mask, "t": t, "taps": taps, "ref": ref}


def _prec(S, prec):
    return {"bf16x3": S.PREC_BF16X3, "f16f8": S.PREC_F16F8}[prec]


def _forward(S, dev, case, prec, conv_ws, keep):
    plan = S.Plan(keep_intermediates=keep, conv_ws=conv_ws, precision=_prec(S, prec))
    blob = plan.pack(case["sd"], dev)
    out = plan.estimator_forward(blob, case["z"].to(dev), case["mask"].to(dev), case["mu"].to(dev), case["t"].to(dev))
    torch.cuda.synchronize()
    return plan, out.cpu()


def _check_finite(tag, plan, out, prec):
    """The estimator output is finite (bf16x3: every utterance), or the format's range limit is on record (f16f8: module docstring)."""
    fin = [bool(torch.isfinite(out[b]).all()) for b in range(B)]
    ev, mx = plan.range_status()
    print("%s | estimator output finite per utterance: %s, range_status: %d events, max |x| %g" % (tag, fin, ev, mx))
    if prec == "f16f8":
        assert fin[:2] == [True, True], fin
        assert ev > 0 and mx == float("inf"), (ev, mx)
    else:
        assert fin == [True] * B, fin


def _regions(lengths, Ho, Wo):
    """Boolean [B][Ho][Wo] maps: first output row; first and last output column; the two output columns on either side of each
    utterance end; everything else."""
    nb = len(lengths)
    row0 = torch.zeros(nb, Ho, Wo, dtype=torch.bool)
    row0[:, 0, :] = True
    cols = torch.zeros(nb, Ho, Wo, dtype=torch.bool)
    cols[:, :, 0] = True
    cols[:, :, Wo - 1] = True
    ends = torch.zeros(nb, Ho, Wo, dtype=torch.bool)
    for b, L in enumerate(lengths):
        oe = (int(L) + 1) // 2          # first output column whose centre tap lies behind the utterance
        for ox in range(oe - 2, oe + 2):
            if 0 <= ox < Wo:
                ends[b, :, ox] = True
    interior = ~(row0 | cols | ends)
    return {"first row": row0, "first/last column": cols, "utterance ends": ends, "interior": interior}


def _check_regions(tag, got, want, lengths):
    scale = float(want.abs().max())
    worst = 0.0
    for name, sel in _regions(lengths, got.shape[2], got.shape[3]).items():
        sel4 = sel[:, None].expand_as(got)
        e = float((got - want)[sel4].abs().max()) / scale
        print("%s | %-17s max|err| / max|ref| = %.3e" % (tag, name, e))
        worst = max(worst, e)
    return worst


@kernels
@precs
def test_folded_downsample_local_and_oracle(S, dev, case, prec, conv_ws):
    """downs.0.3.out of a keep_intermediates plan (the folded Downsample, as in every plan) against F.conv2d on the HIP path's own
    apply output downs.0.2.out, and against the oracle's tap, by region."""
    plan, out = _forward(S, dev, case, prec, conv_ws, keep=True)
    hip = {k: v.detach().cpu().clone() for k, v in plan.tensors(B, T, dev).items()}
    sd, taps = case["sd"], case["taps"]
    m = case["mask"].unsqueeze(1)
    got = hip["downs.0.3.out"]
    local = F.conv2d(hip["downs.0.2.out"] * m, sd["downs.0.3.conv.weight"], sd["downs.0.3.conv.bias"], stride=2, padding=1)
    tag = "%s %s" % (prec, "conv_ws" if conv_ws else "conv_mfma")
    e_att = float((hip["downs.0.2.out"] - taps["downs.0.2.out"]).abs().max() / taps["downs.0.2.out"].abs().max())
    print("%s | attention apply output vs oracle: %.3e" % (tag, e_att))
    e_local = _check_regions(tag + " | local ", got, local, LENGTHS)
    e_oracle = _check_regions(tag + " | oracle", got, taps["downs.0.3.out"], LENGTHS)
    assert e_att <= REL
    assert e_local <= REL, e_local
    assert e_oracle <= REL, e_oracle
    _check_finite(tag, plan, out, prec)


@kernels
@precs
def test_normal_and_keep_intermediates_plans_return_the_same_bits(S, dev, case, prec, conv_ws):
    plan_n, out_n = _forward(S, dev, case, prec, conv_ws, keep=False)
    _, out_k = _forward(S, dev, case, prec, conv_ws, keep=True)
    _check_finite("%s %s" % (prec, "conv_ws" if conv_ws else "conv_mfma"), plan_n, out_n, prec)
    assert torch.equal(out_n.view(torch.int32), out_k.view(torch.int32))      # the same BITS (a NaN is not equal to itself)


@precs
def test_op_report_lists_the_folded_apply(S, prec):
    plan = S.Plan(precision=_prec(S, prec))
    applies = {label: kern for label, kern, _, _ in plan.ops(B, T) if label.endswith(".apply")}
    assert len(applies) == 6, applies
    fused = sorted(label for label, kern in applies.items() if kern.startswith("(fused"))
    assert fused == ["downs.0.2.apply"], applies
    assert applies["downs.0.2.apply"] == "(fused into downs.0.3)"


@precs
def test_diffvc_dim64_folded_downsample(S, dev, prec):
    """DiffVC (arch 1) has the same single-reader structure at level 0: the same local check, inputs of tests/test_gpu_diffvc.py."""
    g = golden("vc_dim64.npz")
    sd = V.make_state(dim_base=64, dim_cond=128, use_ref_t=True, seed=int(g["seed"]), rezero_g=1.0)
    plan = S.Plan(dim=64, arch=1, keep_intermediates=True, precision=_prec(S, prec))
    blob = plan.pack(sd, dev)
    a = [torch.from_numpy(np.asarray(g[k])) for k in ("z", "mask", "mean", "xt_ref", "ref_mask", "c", "t")]
    out = plan.vc_estimator_forward(blob, *[v.to(dev) for v in a]).cpu()
    taps = {}
    ref = V.estimator_forward(sd, *a, taps=taps)
    nb, _, Tv = a[0].shape
    ws, info = plan.vc_tensors(nb, Tv, int(a[4].shape[-1]), dev)

    def view(name):
        off, dims = info[name]
        n = int(np.prod(dims))
        return ws[off: off + 4 * n].view(torch.float32).view(*dims).cpu()

    m = a[1].view(nb, 1, 1, Tv)
    lengths = [int(v) for v in a[1].view(nb, Tv).sum(-1)]
    got = view("downs.0.3.out")
    local = F.conv2d(view("downs.0.2.out") * m, sd["downs.0.3.conv.weight"], sd["downs.0.3.conv.bias"], stride=2, padding=1)
    e_local = _check_regions("diffvc %s | local " % prec, got, local, lengths)
    e_oracle = _check_regions("diffvc %s | oracle" % prec, got, taps["downs.0.3.out"], lengths)
    assert e_local <= REL, e_local
    assert e_oracle <= REL, e_oracle
    assert float((out - ref).abs().max() / ref.abs().max()) <= REL
