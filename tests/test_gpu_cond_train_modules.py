"""GPU tests (-m gpu) of the DiffVC decoder's condition path under training as the modules run it (diffvc/model/modules.py: RefBlock;
diffvc/model/diffusion.py: GradLogPEstimator._first_resnet) at dim_base 64, dim_cond 128, B = 2, T = 36, T_ref = 20, ragged masks:

  autograd   RefBlock and _first_resnet against the same module in float64 on the CPU (stock torch ops): every output and parameter
             gradient within 2e-4 of the tensor's largest element, the bound of tests/test_gpu_diffvc_training.py; a conv bias in front
             of an InstanceNorm (an identically-zero gradient) on the scale of the same layer's weight gradient, as that file does
  conv2d     one loss_t + backward with torch.nn.functional.conv2d replaced by a recorder: the step's calls are exactly RefBlock's
             narrow convolutions listed in _train_ops.COND_LEFT_ON_TORCH -- never final_conv (pooled first), never the condition
             columns (on the trunk's MFMA kernels)
  counters   op_counts() reports no fallback and no fewer HIP ops than before; cond_op_counts() matches the module tree"""
import copy
import importlib

import pytest
import torch

from oracle import diffvc_oracle as V
from gpu_guards import S, dev  # noqa: F401

pytestmark = pytest.mark.gpu
BOUND = 2e-4
DIM, DIM_COND, B, T, T_REF = 64, 128, 2, 36, 20


def _mods():
    return (importlib.import_module("speech-backbones_amd.diffvc.model.diffusion"), importlib.import_module("speech-backbones_amd.model._train_ops"))


def _decoder():
    DV, _ = _mods()
    dec = DV.Diffusion(80, DIM, DIM_COND, True, 0.05, 20.0)
    dec.estimator.load_state_dict(V.make_state(dim_base=DIM, dim_cond=DIM_COND, use_ref_t=True, seed=11, rezero_g=0.3), strict=True)
    return dec


def _mask(lens, n):
    return (torch.arange(n)[None, :] < torch.tensor(lens)[:, None]).float()[:, None]           # [B, 1, n]


def _compare(what, got, ref, scales=None):
    """Worst max |got - ref| / max |ref| over the named tensors (scales: another tensor's scale for some names)."""
    worst = ("", 0.0)
    for n in ref:
        assert (got[n] is None) == (ref[n] is None), (what, n)
        if ref[n] is None:
            continue
        scale = float(ref[(scales or {}).get(n, n)].abs().max())
        e = float((got[n].detach().double().cpu() - ref[n]).abs().max()) / (scale + 1e-30)
        worst = max(worst, (n, e), key=lambda kv: kv[1])
    print("%s GPU vs float64 CPU autograd: worst %.2e (%s)" % (what, worst[1], worst[0]))
    assert worst[1] <= BOUND, (what, worst)


def test_refblock_under_autograd_matches_float64(S, dev):
    _, TO = _mods()
    g = torch.Generator().manual_seed(21)
    rb = _decoder().estimator.ref_block
    x, temb, dout = torch.randn(B, 1, 80, T_REF, generator=g), torch.randn(B, DIM, generator=g), torch.randn(B, DIM_COND, generator=g)
    mask = _mask([T_REF, 13], T_REF)[:, None]                                                   # [B, 1, 1, T_ref]
    cpu = copy.deepcopy(rb).double()
    tc = temb.double().requires_grad_(True)
    oc = cpu(x.double(), mask.double(), tc)
    oc.backward(dout.double())
    ref = dict({n: p.grad for n, p in cpu.named_parameters()}, out=oc.detach(), dtemb=tc.grad)
    gpu = rb.to(dev)
    tg = temb.to(dev).requires_grad_(True)
    importlib.import_module("speech-backbones_amd")._lib.new_pack_generation()
    TO.reset_op_counts()
    TO.reset_cond_op_counts()
    og = gpu(x.to(dev), mask.to(dev), tg)
    og.backward(dout.to(dev))
    got = dict({n: p.grad for n, p in gpu.named_parameters()}, out=og, dtemb=tg.grad)
    scales = {n: n[:-len("bias")] + "weight" for n in ref if n.startswith("block") and n.endswith(".0.bias")}
    _compare("RefBlock", got, ref, scales)
    left = sum((blk[0].in_channels, blk[0].out_channels) in TO.COND_LEFT_ON_TORCH for blk in (gpu.block11, gpu.block12, gpu.block21))
    assert TO.cond_op_counts() == (3 + (3 - left), left), TO.cond_op_counts()                    # 2 time-bias adds, the pool, the narrow layers
    assert TO.op_counts()[1] == 0


def test_first_resnet_under_autograd_matches_float64(S, dev):
    _, TO = _mods()
    g = torch.Generator().manual_seed(22)
    est = _decoder().estimator
    v2, cond, temb = torch.randn(B, 2, 80, T, generator=g), torch.randn(B, DIM_COND, generator=g), torch.randn(B, DIM, generator=g)
    dout = torch.randn(B, DIM, 80, T, generator=g)
    m = _mask([T, 23], T)[:, None]
    cpu = copy.deepcopy(est).double()
    cc, tc = cond.double().requires_grad_(True), temb.double().requires_grad_(True)
    oc = cpu._first_resnet(cpu.downs[0][0], v2.double(), cc[:, :, None, None].expand(-1, -1, 80, T).contiguous(), m.double(), tc)
    oc.backward(dout.double())
    ref = dict({n: p.grad for n, p in cpu.downs[0][0].named_parameters()}, out=oc.detach(), dcond=cc.grad, dtemb=tc.grad)
    gpu = est.to(dev)
    cg, tg = cond.to(dev).requires_grad_(True), temb.to(dev).requires_grad_(True)
    importlib.import_module("speech-backbones_amd")._lib.new_pack_generation()
    TO.reset_op_counts()
    TO.reset_cond_op_counts()
    og = gpu._first_resnet(gpu.downs[0][0], v2.to(dev), cg[:, :, None, None].expand(-1, -1, 80, T).contiguous(), m.to(dev), tg)
    og.backward(dout.to(dev))
    got = dict({n: p.grad for n, p in gpu.downs[0][0].named_parameters()}, out=og, dcond=cg.grad, dtemb=tg.grad)
    _compare("_first_resnet", got, ref)
    assert TO.op_counts()[1] == 0, TO.op_counts()


def _step(dec, dev, record=None):
    g = torch.Generator().manual_seed(23)
    x0, mean, xr, mr = (torch.randn(B, 80, T, generator=g).to(dev) for _ in range(4))
    c = (torch.randn(B, 256, generator=g) * 0.3).to(dev)
    mask = _mask([T, 23], T).to(dev)
    t = torch.tensor([0.3, 0.8], device=dev)
    torch.manual_seed(5)
    F = torch.nn.functional
    orig = F.conv2d

    def recorder(inp, weight, *a, **k):
        record.append((int(weight.shape[1]), int(weight.shape[0]), int(weight.shape[2])))
        return orig(inp, weight, *a, **k)
    if record is not None:
        F.conv2d = recorder
    try:
        loss = dec.loss_t(x0, mask, mean, xr, mr, c, t)
        loss.backward()
    finally:
        F.conv2d = orig
    return float(loss.detach())


def test_one_training_step_calls_conv2d_only_for_the_layers_left_on_torch(S, dev):
    _, TO = _mods()
    dec = _decoder().to(dev)
    rb = dec.estimator.ref_block
    narrow = [(blk[0].in_channels, blk[0].out_channels) for blk in (rb.block11, rb.block12, rb.block21)]
    assert narrow == [(1, 64), (32, 64), (32, 128)]
    assert all(k in narrow for k in TO.COND_LEFT_ON_TORCH), "only RefBlock's narrow convolutions may be listed"
    predicted = sorted((ci, co, 3) for ci, co in narrow if (ci, co) in TO.COND_LEFT_ON_TORCH)
    calls = []
    TO.reset_op_counts()
    TO.reset_cond_op_counts()
    loss = _step(dec, dev, calls)
    print("conv2d calls of one DiffVC training step at dim %d: %s (COND_LEFT_ON_TORCH %s)" % (DIM, sorted(calls), sorted(TO.COND_LEFT_ON_TORCH)))
    assert loss == loss and sorted(calls) == predicted, (sorted(calls), predicted)
    hip_ops, fallbacks = TO.op_counts()
    print("op_counts %s, cond_op_counts %s" % ((hip_ops, fallbacks), TO.cond_op_counts()))
    assert fallbacks == 0 and hip_ops >= 54, (hip_ops, fallbacks)
    # the module tree: 3 narrow convolutions, 2 time-bias adds, 1 pool; the fallbacks are the layers left on torch
    assert TO.cond_op_counts() == (6 - len(predicted), len(predicted)), TO.cond_op_counts()
