"""GPU tests (-m gpu) of the train.py step, GradTTS.compute_loss + backward with the encoder attached: the prior mean mu_y comes from the
encoder, so the decoder's first layer needs a data gradient (gtts_conv_dgrad_small), the noising runs under autograd
(gtts_diffusion_noising_backward) and the alignment glue between MAS and the decoder runs on csrc/glue_train.hip.

  1, 2   single- and multi-speaker, without a crop and with out_size = 48 and one y_length below it: zero torch fallbacks among the
         decoder ops, the three glue ops counted, losses within 2e-4 and every parameter gradient within 5e-4 of the same module on the
         CPU (the bounds and the conv_k.bias / scalar rules of tests/test_gpu_training.py::test_gradtts_compute_loss_multispeaker_gpu_vs_cpu)
  3      under FORCE_TORCH the same step runs the torch composition: the glue counters do not move
  4      Diffusion.compute_loss with a mu that does not require grad is bit-equal before and after a call whose mu does
Dropout is off (eval mode), t and z are drawn once and replayed on both sides, y holds every token's own prior mean for its share of the
frames so that MAS is unambiguous, and Python's `random` is seeded alike on both sides."""
import copy
import functools
import importlib
import random

import pytest
import torch
from case_util import relerr_floor as relerr

pytestmark = pytest.mark.gpu
B, TX, T = 3, 17, 64
X_LENGTHS, Y_LENGTHS = (17, 11, 14), (64, 48, 40)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def setup(n_spks):
    """(cpu model, inputs): built once per speaker count, never modified (the tests work on deep copies)."""
    M = importlib.import_module("speech-backbones_amd.model")
    torch.manual_seed(3 + n_spks)
    cpu = M.GradTTS(149, n_spks, 64, 192, 768, 256, 2, 6, 3, 0.1, 4, 80, 64, 0.05, 20.0, 1000).eval()      # (dropout off: deterministic)
    with torch.no_grad():
        for n, prm in cpu.decoder.estimator.named_parameters():
            if n.endswith("fn.g"):
                prm.fill_(0.3)
        cpu.encoder.proj_m.weight.mul_(8.0)
        cpu.encoder.proj_m.bias.mul_(8.0)
    g = torch.Generator().manual_seed(4)
    x = torch.randint(0, 149, (B, TX), generator=g)
    xl, yl = torch.tensor(X_LENGTHS), torch.tensor(Y_LENGTHS)
    spk = torch.tensor([1, 4, 2]) if n_spks > 1 else None
    with torch.no_grad():
        mu_x, _, _ = cpu.encoder(x, xl, cpu.spk_emb(spk) if n_spks > 1 else None)
    y = torch.zeros(B, 80, T)
    for b in range(B):
        edges = torch.linspace(0, int(yl[b]), int(xl[b]) + 1).round().long()
        for j in range(int(xl[b])):
            y[b, :, edges[j]:edges[j + 1]] = mu_x[b, :, j:j + 1]
    y = (y + 0.05 * torch.randn(B, 80, T, generator=g)) * (torch.arange(T)[None, None, :] < yl[:, None, None])
    return cpu, dict(x=x, xl=xl, y=y, yl=yl, spk=spk, t=torch.tensor([0.37, 0.71, 0.12]), z={s: torch.randn(B, 80, s, generator=g) for s in (T, 48)})


def step(model, inp, d, out_size):
    """compute_loss + backward with t and z replayed and `random` seeded; returns the three losses as floats."""
    t_fix, z_fix = inp["t"], inp["z"][T if out_size is None else out_size]
    orig_rand, orig_randn = torch.rand, torch.randn
    torch.rand = lambda *a, **k: t_fix.to(k.get("device", "cpu"))
    torch.randn = lambda *a, **k: z_fix.to(k.get("device", "cpu"))
    random.seed(11)
    try:
        losses = model.compute_loss(inp["x"].to(d), inp["xl"].to(d), inp["y"].to(d), inp["yl"].to(d),
                                    spk=None if inp["spk"] is None else inp["spk"].to(d), out_size=out_size)
    finally:
        torch.rand, torch.randn = orig_rand, orig_randn
    sum(losses).backward()
    return [float(v.detach()) for v in losses]


@functools.lru_cache(maxsize=None)
def cpu_step(n_spks, out_size):
    cpu0, inp = setup(n_spks)
    cpu = copy.deepcopy(cpu0)
    losses = step(cpu, inp, torch.device("cpu"), out_size)
    return cpu, losses


def compare_gradients(cpu, gpu):
    worst = ("", 0.0)
    pc = dict(cpu.named_parameters())
    for name, p in gpu.named_parameters():
        if p.grad is None or pc[name].grad is None:
            assert (p.grad is None) == (pc[name].grad is None), name
            continue
        if name.endswith("conv_k.bias"):
            # d loss / d (key bias) is identically zero: both sides hold rounding noise only, measured against the layer's weight gradient
            ref = float(pc[name[:-4] + "weight"].grad.abs().max())
            assert float(p.grad.abs().max()) <= 1e-4 * ref and float(pc[name].grad.abs().max()) <= 1e-4 * ref, name
            continue
        e = relerr(p.grad.cpu(), pc[name].grad)
        if p.numel() == 1:
            e = e / 5.0
        worst = max(worst, (name, e), key=lambda kv: kv[1])
    return worst


@pytest.mark.parametrize("out_size", [None, 48])
@pytest.mark.parametrize("n_spks", [1, 5])
def test_train_step_runs_on_the_kernels_and_matches_the_cpu(dev, n_spks, out_size):
    TO = importlib.import_module("speech-backbones_amd.model._train_ops")
    cpu0, inp = setup(n_spks)
    cpu, lc = cpu_step(n_spks, out_size)
    gpu = copy.deepcopy(cpu0).to(dev)
    TO.reset_op_counts(), TO.reset_enc_op_counts(), TO.reset_glue_op_counts()
    lg = step(gpu, inp, dev, out_size)
    hip_ops, fallbacks = TO.op_counts()
    print("GradTTS(%d).compute_loss out_size=%s: decoder ops %s, encoder ops %s, glue ops %s" % (n_spks, out_size, TO.op_counts(),
                                                                                               TO.enc_op_counts(), TO.glue_op_counts()))
    assert fallbacks == 0 and hip_ops >= 54, (hip_ops, fallbacks)          # the first layer's two convolutions fell back before
    assert TO.glue_op_counts() == (3, 0)                                    # path index, duration loss, crop / gather / prior loss
    assert TO.enc_op_counts()[1] == 0
    for a, b, name in zip(lc, lg, ("duration", "prior", "diffusion")):
        print("  %-9s cpu %.7f gpu %.7f rel %.2e" % (name, a, b, abs(a - b) / abs(a)))
        assert abs(a - b) <= 2e-4 * abs(a) + 1e-6, (name, a, b)
    worst = compare_gradients(cpu, gpu)
    print("  worst gradient rel err %.2e (%s)" % worst[::-1])
    assert worst[1] <= 5e-4, worst
    for name in ("encoder.proj_m.weight", "encoder.proj_w.proj.weight", "encoder.emb.weight"):
        assert float(dict(gpu.named_parameters())[name].grad.abs().max()) > 0, name     # the encoder is reached through mu_y and logw
    if n_spks > 1:
        assert gpu.spk_emb.weight.grad is not None and float(gpu.spk_emb.weight.grad.abs().max()) > 0
        assert relerr(gpu.spk_emb.weight.grad.cpu(), cpu.spk_emb.weight.grad) <= 5e-4


def test_force_torch_runs_the_composition(dev):
    """The measurement switch routes the same step to the dense torch composition: no glue op is counted, and the two deterministic
    losses agree with the kernel path.  Both sides start from fp32 encoder outputs of different implementations, so the agreement is
    held to the cap of the per-op bound, 1e-4."""
    TO = importlib.import_module("speech-backbones_amd.model._train_ops")
    cpu0, inp = setup(1)
    res = {}
    for force in (False, True):
        gpu = copy.deepcopy(cpu0).to(dev)
        TO.reset_glue_op_counts(), TO.reset_op_counts()
        TO.FORCE_TORCH = force
        try:
            res[force] = step(gpu, inp, dev, 48)
        finally:
            TO.FORCE_TORCH = False
        assert TO.glue_op_counts() == ((0, 0) if force else (3, 0)), (force, TO.glue_op_counts())
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for n, p in gpu.named_parameters() if not n.startswith("spk_emb"))
    for a, b, name in zip(res[True], res[False], ("duration", "prior")):
        print("%-9s torch %.7f kernels %.7f rel %.2e" % (name, a, b, abs(a - b) / abs(a)))
        assert abs(a - b) <= 1e-4 * abs(a), (name, a, b)


def test_decoder_only_training_is_untouched(dev):
    """Diffusion.compute_loss with a prior mean that carries no gradient takes the plain noising kernel (never the autograd Function),
    and gives the same bits before and after a call whose mu requires grad."""
    D = importlib.import_module("speech-backbones_amd.model.diffusion")
    TO = importlib.import_module("speech-backbones_amd.model._train_ops")
    from oracle import gradtts_oracle as O
    dec = D.Diffusion(80, 64, 1, 64, 0.05, 20.0, 1000)
    dec.estimator.load_state_dict(O.make_estimator_state(seed=4, rezero_g=0.3), strict=True)
    dec = dec.to(dev)
    inp = O.make_inputs(2, 64, seed=8)
    x0, mask, mu = (inp[k].to(dev) for k in ("z", "mask", "mu"))
    calls = []
    orig = TO.Noising.apply

    def run(mu_in):
        dec.zero_grad(set_to_none=True)
        torch.manual_seed(0)
        TO.Noising.apply = lambda *a: (calls.append(1), orig(*a))[1]
        try:
            loss, _ = dec.compute_loss(x0, mask, mu_in)
        finally:
            TO.Noising.apply = orig
        loss.backward()
        return loss.detach().clone(), [p.grad.clone() for p in dec.parameters()]

    l0, g0 = run(mu)
    assert not calls
    mu_g = mu.clone().requires_grad_(True)
    l1, _ = run(mu_g)
    assert calls and mu_g.grad is not None and float(mu_g.grad.abs().max()) > 0 and abs(float(l1) - float(l0)) <= 1e-6 * abs(float(l0))
    n = len(calls)
    l2, g2 = run(mu)
    assert len(calls) == n
    assert torch.equal(l0, l2) and all(torch.equal(a, b) for a, b in zip(g0, g2))
