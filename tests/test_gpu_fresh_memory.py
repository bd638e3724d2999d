"""GPU tests (-m gpu): no result depends on what fresh memory held (include/gradtts_abi.h: workspace, scratch, saved-state and output
buffers may hold any bytes on entry).

Every buffer the package hands to the library comes from torch.empty / torch.empty_like.  tests/alloc_poison.py replaces the two so that
every such tensor on the device lies over 0x00000000, then 0xFFFFFFFF (NaN, -1, fp8 0xFF), 0x7F800000 (+Inf) and 0xFF7FFFFF (-FLT_MAX),
and each case below -- one per family of entry points -- builds its plan or module, packs, uploads its inputs and calls, once per pattern:
every returned tensor must be finite and have the bits of the all-zero run.  No bound here is a measured number; the accuracy of the
all-zero run is held by the parity suites.  Shapes are the smallest the existing suites name for each mechanism (ragged batches, a length
of 1, one element past a tile); injected randomness (noise, t, dropout seeds) is fixed per closure.

A bit-for-bit comparison can only hold arithmetic that repeats.  The package's kernels do; the framework's own convolution does not (on
an MI355X two GradTTS.compute_loss steps on the same inputs over the SAME fill differed in 294 of 308 gradients, two DiffVC loss_t steps in
the three weight gradients of RefBlock's narrow layers -- exactly the layers model/_train_ops.py leaves on torch.nn.functional.conv1d /
conv2d by measurement: ENC_CONV_LEFT_ON_TORCH, the forward of ENC_CONV_KERNEL_FORWARD, COND_LEFT_ON_TORCH).  The training cases therefore
switch those layers to the package's kernels, as tests/test_gpu_enc_conv_train_modules.py and tests/test_gpu_cond_train_modules.py do, and
assert that no op fell back: every convolution of the step then runs on a buffer this package allocated.

The inputs avoid the two results that are NaN by design: a silent row under normalize(increase_only), an all-zero speaker embedding."""
import copy
import importlib
import os

import numpy as np
import pytest
import torch

import alloc_poison as AP
import fgl_oracle as FO
import ge2e_oracle as GO
import mel_oracle as MO
import spk_oracle as SO
import wav_oracle as WO
from case_util import seq_mask
from gpu_guards import L, S, dev  # noqa: F401
from oracle import diffvc_oracle as V
from oracle import encoder_oracle as E
from oracle import gradtts_oracle as O
from oracle import postnet_oracle as PO

pytestmark = pytest.mark.gpu
PKG = "speech-backbones_amd"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG2048 = (2048, 80, 22050, 512)        # the largest Griffin-Lim transform (tests/test_gpu_fgl.py)


def _mod(name):
    return importlib.import_module(PKG + name)


@pytest.fixture
def fresh(L, dev, monkeypatch):
    """fresh(family, shape, closure): alloc_poison.check on this device, with every cache of the package dropped before each pattern."""
    def reset():
        L.clear_packed_cache()
        L._CONSTS.clear()
        L._GE2E_WS.clear()
        for name in (".hifi_gan.meldataset", ".diffvc.model.utils", ".diffvc.speaker_encoder.encoder.audio"):
            _mod(name)._blobs.clear()
        torch.cuda.synchronize()

    def go(family, shape, closure):
        return AP.check(closure, monkeypatch, dev, family=family, shape=str(shape), reset=reset)
    return go


def _replayed(noise, call, rand=None):
    """call() with torch.randn (and torch.rand) returning the given tensors: how the training suites inject the noise and t draws."""
    orig = torch.randn, torch.rand
    torch.randn = lambda *a, **k: noise.to(k.get("device", "cpu"))
    if rand is not None:
        torch.rand = lambda *a, **k: rand.to(k.get("device", "cpu"))
    try:
        return call()
    finally:
        torch.randn, torch.rand = orig


def _param_grads(module, prefix="d "):
    return {prefix + n: p.grad for n, p in module.named_parameters() if p.grad is not None}


def _same(a, b, what):
    assert torch.equal(a.reshape(-1).view(torch.int32), b.reshape(-1).view(torch.int32)), what


# =============================================================================================================== inference
@pytest.mark.parametrize("prec", ["bf16x3", "f16f8"])
def test_diffvc_plan(S, dev, fresh, prec):
    """dim 64, B = 3 ragged, T = 100, T_ref = 72: the estimator, and two sampler steps in each mode with injected noise.  Then the sequence
    that exposed the round-6 halo read: a call that overflows (inputs x 1000) leaves NaN in the workspace, and the normal call after it
    on the same plan must return the bits of a normal call on a fresh one."""
    precision = {"bf16x3": S.PREC_BF16X3, "f16f8": S.PREC_F16F8}[prec]
    sd = V.make_state(dim_base=64, dim_cond=128, use_ref_t=True, seed=2)
    inp = V.make_inputs(3, 100, 72, seed=4)
    t = torch.tensor([0.75, 0.3, 0.5])
    xt_ref = torch.stack([V.compute_diffused_mean(inp["ref"], inp["ref_mask"], inp["mean_ref"], 0.6)], 1)
    noise = torch.randn(2, 3, 80, 100, generator=torch.Generator().manual_seed(5))

    def setup():
        plan = S.Plan(dim=64, arch=1, precision=precision)
        return plan, plan.pack(sd, dev), {k: v.to(dev) for k, v in inp.items()}

    def est(plan, blob, a, scale=1.0):
        return plan.vc_estimator_forward(blob, a["z"] * scale, a["mask"], a["mean"] * scale, xt_ref.to(dev) * scale, a["ref_mask"], a["c"], t.to(dev))

    def run():
        plan, blob, a = setup()
        out = {"est": est(plan, blob, a)}
        for mode in ("pf", "em", "ml"):
            out[mode] = plan.vc_reverse_diffusion(blob, a["z"], a["mask"], a["mean"], a["ref"], a["ref_mask"], a["mean_ref"], a["c"], 2, mode,
                                                  noise=None if mode == "pf" else noise.to(dev))
        return out

    def after_an_overflow():
        plan, blob, a = setup()
        est(plan, blob, a, 1000.0)
        return {"est": est(plan, blob, a)}

    base = fresh("DiffVC Plan " + prec, "dim 64 B 3 T 100 T_ref 72", run)
    seq = fresh("DiffVC Plan " + prec + " after overflow", "dim 64 B 3 T 100 T_ref 72", after_an_overflow)
    _same(seq["est"], base["est"], "the call after an overflowing one differs from a call on a fresh plan")


@pytest.mark.parametrize("prec", ["bf16", "bf16_store"])
def test_gradtts_plan(S, dev, fresh, prec):
    """The two precisions tests/test_gpu_range.py leaves out, with speakers: the estimator and a 2-step sampler at B = 3 ragged, T = 100,
    and the sampler as a replayed hipGraph at B = 1."""
    precision = {"bf16": S.PREC_BF16, "bf16_store": S.PREC_BF16_STORE}[prec]
    sd = O.make_estimator_state(n_spks=3, seed=2)
    inp = O.make_inputs(3, 100, seed=4, ragged=True, spk_dim=64)
    t = torch.tensor([0.75, 0.3, 0.5])
    noise = torch.randn(2, 3, 80, 100, generator=torch.Generator().manual_seed(6))

    def run():
        plan = S.Plan(n_spks=3, precision=precision)
        blob = plan.pack(sd, dev)
        z, m, mu, spk = (inp[k].to(dev) for k in ("z", "mask", "mu", "spk"))
        out = {"est": plan.estimator_forward(blob, z, m, mu, t.to(dev), spk),
               "ode": plan.reverse_diffusion(blob, z, m, mu, 2, spk),
               "sde": plan.reverse_diffusion(blob, z, m, mu, 2, spk, noise=noise.to(dev))}
        graph = S.Plan(n_spks=3, precision=precision)
        graph.set_graph(True)
        gblob = graph.pack(sd, dev)
        out["graph first"] = graph.reverse_diffusion(gblob, z[:1], m[:1], mu[:1], 2, spk[:1])
        out["graph replay"] = graph.reverse_diffusion(gblob, z[:1], m[:1], mu[:1], 2, spk[:1])
        return out

    base = fresh("Grad-TTS Plan " + prec, "dim 64 3 speakers B 3 T 100; graph B 1", run)
    _same(base["graph first"], base["graph replay"], "the replayed graph differs from its first launch")


@pytest.mark.parametrize("mode", ["text", "mel"])
def test_encoder(S, dev, fresh, mode):
    """B = 3, lengths (129, 64, 1): L crosses one time tile, one sample is a single position."""
    Lx, lens = 129, (129, 64, 1)
    sd = E.make_state(mode, seed=7)
    g = torch.Generator().manual_seed(8)
    x = torch.randint(0, 149, (3, Lx), generator=g) if mode == "text" else torch.randn(3, 80, Lx, generator=g)
    mask = seq_mask(lens, Lx).unsqueeze(1)

    def run():
        enc = S.Encoder("text") if mode == "text" else S.Encoder("mel", 0, 80, 192, 768, 0, 2, 6, 3, 4)
        out = enc.forward(enc.pack(sd, dev), x.to(dev), mask.to(dev))
        return dict(mu=out[0], logw=out[1]) if mode == "text" else dict(out=out)

    fresh("Encoder " + mode, "B 3 L 129 lengths (129, 64, 1)", run)


def test_conv1d_op_with_pad_channels(S, dev, fresh):
    """cin 20 and cout 24: a partial channel chunk (the pad channels of conv1d.h must read 0 whatever follows the sample in memory) and a
    partial row tile; the forward, and the weight gradient with its workspace from torch.empty."""
    B, cin, cout, K, Lx, lens = 3, 20, 24, 3, 129, (129, 64, 1)
    g = torch.Generator().manual_seed(9)
    x, dy = torch.randn(B, cin, Lx, generator=g), torch.randn(B, cout, Lx, generator=g)
    w = (torch.rand(cout, cin, K, generator=g) * 2 - 1) / (cin * K) ** 0.5
    bias = torch.rand(cout, generator=g) - 0.5
    mask = seq_mask(lens, Lx)

    def run():
        op = S.Conv1dOp(0, cin, cout, K)
        xd, m = x.to(dev), mask.to(dev)
        y = op.forward(op.pack(w, dev), bias.to(dev), xd, in_mask=m, out_mask=m)
        dw, db = op.wgrad(xd, dy.to(dev), in_mask=m, out_mask=m)
        return dict(y=y, dw=dw, db=db)

    fresh("Conv1dOp forward + wgrad", "cin 20 cout 24 K 3 B 3 L 129", run)


def test_postnet_plan(S, dev, fresh):
    sd = PO.make_state(128, seed=0)
    x = torch.randn(2, 80, 37, generator=torch.Generator().manual_seed(37))
    mask = seq_mask((37, 18), 37).unsqueeze(1)

    def run():
        plan = S.PostNetPlan(128)
        return plan.forward(plan.pack(sd, dev), x.to(dev), mask.to(dev))

    fresh("PostNetPlan.forward", "dim 128 B 2 T 37 lengths (37, 18)", run)


def test_mel_plan_forward_and_backward(S, dev, fresh):
    """B = 3 with lengths, 19 frames: three past the forward's tile of 16."""
    Lw, lens = 256 * 19, (256 * 19, 845, 385)
    y = MO.signal("speechlike", Lw)[:3]
    dmel = torch.randn(3, 80, 19, generator=torch.Generator().manual_seed(19))

    def run():
        plan = S.MelPlan(*MO.CFG1)
        blob = plan.pack(dev)
        n = torch.tensor(lens, dtype=torch.int32, device=dev)
        return dict(mel=plan.forward(blob, y.to(dev), n), dwav=plan.backward(blob, y.to(dev), dmel.to(dev), n),
                    mel_full=plan.forward(blob, y.to(dev)), dwav_full=plan.backward(blob, y.to(dev), dmel.to(dev)))

    fresh("MelPlan forward + backward", "cfg1 B 3 L %d lengths %s" % (Lw, lens), run)


@pytest.mark.parametrize("tag,cfg,T", [("cfgA", FO.CFGA, 17), ("n2048", CFG2048, 19)])
def test_fgl_plan(S, dev, fresh, tag, cfg, T):
    """init, one step from the zero phase, forward(n = 2); B = 2.  The 2-step waveform is compared with itself bit for bit."""
    inv = FO.basis64(cfg)[1].float()
    s = FO.logmel("speechlike", cfg, T)[:2]

    def run():
        plan = S.FglPlan(cfg[0], cfg[1], cfg[3], FO.MOMENTUM)
        blob = plan.pack(inv, dev)
        c, x0 = plan.init(blob, s.to(dev))
        x1, a = plan.step(blob, c, x0, torch.zeros(c.shape, dtype=torch.complex64, device=dev))
        return dict(c=c, x0=x0, x1=x1, a=a, wav=plan.forward(blob, s.to(dev), 2))

    fresh("FglPlan " + tag, "B 2 T %d" % T, run)


def test_wav_plan(S, dev, fresh):
    """resample at L = 1412 (1025 outputs: one past its tile), normalize with and without the resampler's partials, powmel; B = 3."""
    x22 = 0.01 * WO.wave("speechlike", 1412, 22050)
    x16 = WO.wave("noise", 160 * 32, 16000)

    def run():
        p = S.WavPlan(22050, 16000)
        blob = p.pack(dev)
        y, partials = p.resample(blob, x22.to(dev))
        return dict(resampled=y, partials=partials, normalized=p.normalize(blob, y, -30, increase_only=True, partials=partials),
                    normalized_alone=p.normalize(blob, y, -30, increase_only=True), powmel=p.powmel(blob, x16.to(dev)))

    base = fresh("WavPlan", "B 3 L 1412 -> 1025; powmel L 5120", run)
    _same(base["normalized"], base["normalized_alone"], "normalize differs with and without the resampler's partials")


def test_spk_plan_forward(S, dev, fresh):
    sd = SO.state("default")
    plain, parts = SO.frames("noise", 17, 160), SO.frames("noise", 2, 400)

    def run():
        plan = S.SpkPlan()
        blob = plan.pack(sd, dev)
        e, h = plan.forward(blob, plain.to(dev), want_hidden=True)
        pe, ph, utt = plan.forward(blob, parts.to(dev), P=4, S=80, T=160, want_hidden=True, want_utt=True)
        return dict(embeds=e, hidden=h, part_embeds=pe, part_hidden=ph, utt=utt)

    fresh("SpkPlan.forward", "(17, 160); P 4 S 80 T 160 on [2, 400, 40]", run)


def _mas_case(b, tx, ty, pairs, seed):
    """value, mask [b, tx, ty] with sample k live on [:t_x, :t_y] = pairs[k]."""
    value = torch.randn(b, tx, ty, generator=torch.Generator().manual_seed(seed))
    mask = torch.zeros(b, tx, ty)
    for k, (t_x, t_y) in enumerate(pairs):
        mask[k, :t_x, :t_y] = 1
    return value, mask


def test_mas_both_kernels(S, dev, fresh):
    """t_x <= 1024 runs the one-wave kernel, t_x = 1025 the column sweep: each on a ragged batch with a full sample, a short one and one
    with more tokens than frames (t_x > t_y: the degenerate walk)."""
    wave = _mas_case(3, 40, 70, [(40, 70), (23, 51), (40, 9)], 1)
    sweep = _mas_case(3, 1025, 1030, [(1025, 1030), (300, 517), (1025, 6)], 2)

    def run():
        return dict(wave=S.mas_maximum_path(wave[0].to(dev), wave[1].to(dev)), sweep=S.mas_maximum_path(sweep[0].to(dev), sweep[1].to(dev)))

    base = fresh("mas_maximum_path", "wave [3, 40, 70]; sweep [3, 1025, 1030]", run)
    for name, (value, mask) in (("wave", wave), ("sweep", sweep)):
        t_y = mask.sum(2)[:, 0]
        assert torch.equal(base[name].sum(1).sum(1), t_y), name          # one token per live frame: the kernels did run a path


def test_host_glue(L, dev, fresh):
    """log_prior, expand_alignment and euler_step (in place, on the z that expand_alignment allocated)."""
    g = torch.Generator().manual_seed(3)
    B, F, tx, T = 3, 80, 17, 70
    mu_x, y = torch.randn(B, F, tx, generator=g), torch.randn(B, F, T, generator=g)
    x_mask = seq_mask((17, 11, 1), tx)
    dur = torch.randint(1, 5, (B, tx), generator=g).float() * x_mask
    y_len = dur.sum(1).long().clamp(max=T)
    noise, est = torch.randn(B, F, T, generator=g), torch.randn(B, F, T, generator=g)
    y_mask = seq_mask(y_len.tolist(), T).unsqueeze(1)

    def run():
        attn, mu_y, z = L.expand_alignment(dur.to(dev), x_mask.to(dev), y_len.to(dev), mu_x.to(dev), T, noise.to(dev), 1.5)
        xt = L.euler_step(z.clone(), mu_y, est.to(dev), y_mask.to(dev), 7.3, 0.1, noise.to(dev))
        return dict(log_prior=L.log_prior(mu_x.to(dev), y.to(dev)), attn=attn, mu_y=mu_y, z=z, xt=xt)

    fresh("log_prior, expand_alignment, euler_step", "B 3 F 80 t_x 17 T 70", run)


# ================================================================================================================ training
def test_gradtts_decoder_training_step(S, dev, fresh):
    """Diffusion.loss_t + backward on the fixture of tests/test_gpu_training.py (tests/golden/loss_grads.npz, one speaker), noise replayed."""
    G = np.load(os.path.join(GOLDEN, "loss_grads.npz"))
    D, TO = _mod(".model.diffusion"), _mod(".model._train_ops")
    sd = O.make_estimator_state(n_spks=1, seed=int(G["s1_seed"]))
    z, mask, mu, t, noise = (torch.from_numpy(G["s1_" + k]) for k in ("z", "mask", "mu", "t", "noise"))

    def run():
        dec = D.Diffusion(80, 64, 1, 64, 0.05, 20.0, 1000)
        dec.estimator.load_state_dict(sd, strict=True)
        dec = dec.to(dev)
        TO.reset_op_counts()
        loss, xt = _replayed(noise, lambda: dec.loss_t(z.to(dev), mask.to(dev), mu.to(dev), t.to(dev), None))
        loss.backward()
        assert TO.op_counts()[1] == 0 and TO.op_counts()[0] >= 54, TO.op_counts()
        return dict(_param_grads(dec.estimator), loss=loss.detach(), xt=xt.detach())

    fresh("Grad-TTS Diffusion.loss_t + backward", "loss_grads.npz s1 %s" % (tuple(z.shape),), run)


def test_gradtts_encoder_decoder_training_step(dev, fresh, monkeypatch):
    """GradTTS.compute_loss + backward (encoder, MAS, the alignment glue, the decoder) on the fixture of tests/test_gpu_tts_train_path.py:
    one speaker, the 48-frame crop; t, the noise and the crop's window draws replayed.  Every encoder convolution on the kernels, forward
    included (the module docstring says why)."""
    import test_gpu_tts_train_path as TP
    TO = _mod(".model._train_ops")
    monkeypatch.setattr(TO, "ENC_CONV_LEFT_ON_TORCH", frozenset())
    monkeypatch.setattr(TO, "ENC_CONV_KERNEL_FORWARD", True)
    cpu0, inp = TP.setup(1)

    def run():
        gpu = copy.deepcopy(cpu0).to(dev)
        TO.reset_op_counts(), TO.reset_enc_op_counts(), TO.reset_enc_conv_op_counts(), TO.reset_glue_op_counts()
        losses = TP.step(gpu, inp, dev, 48)
        assert TO.op_counts()[1] == 0 and TO.enc_op_counts()[1] == 0 and TO.enc_conv_op_counts()[1] == 0 and TO.glue_op_counts() == (3, 0)
        assert TO.enc_conv_op_counts()[0] > 0 and TO.op_counts()[0] >= 54
        return dict(_param_grads(gpu), losses=torch.tensor(losses))

    fresh("GradTTS.compute_loss + backward", "B %d t_x %d T %d crop 48" % (TP.B, TP.TX, TP.T), run)


def test_diffvc_decoder_training_step(S, dev, fresh, monkeypatch):
    """DiffVC Diffusion.loss_t + backward on the d64 fixture of tests/golden/vc_loss_grads.npz: the trunk, RefBlock, the condition field and
    the narrow kernels of csrc/train_narrow.hip (no layer kind left on the framework's convolution: the module docstring says why)."""
    G = np.load(os.path.join(GOLDEN, "vc_loss_grads.npz"))
    DV, TO = _mod(".diffvc.model.diffusion"), _mod(".model._train_ops")
    monkeypatch.setattr(TO, "COND_LEFT_ON_TORCH", frozenset())
    sd = V.make_state(dim_base=64, dim_cond=128, use_ref_t=True, seed=int(G["d64_seed"]), rezero_g=0.3)
    a = {k: torch.from_numpy(G["d64_" + k]) for k in ("x0", "mask", "mean", "x_ref", "mean_ref", "c", "t", "noise")}

    def run():
        dec = DV.Diffusion(80, 64, 128, True, 0.05, 20.0)
        dec.estimator.load_state_dict(sd, strict=True)
        dec = dec.to(dev)
        TO.reset_op_counts(), TO.reset_cond_op_counts()
        loss = _replayed(a["noise"], lambda: dec.loss_t(*[a[k].to(dev) for k in ("x0", "mask", "mean", "x_ref", "mean_ref", "c", "t")]))
        loss.backward()
        assert TO.op_counts()[1] == 0 and TO.cond_op_counts()[1] == 0 and TO.cond_op_counts()[0] >= 3, (TO.op_counts(), TO.cond_op_counts())
        return dict(_param_grads(dec.estimator), loss=loss.detach())

    fresh("DiffVC Diffusion.loss_t + backward", "vc_loss_grads.npz d64 %s" % (tuple(a["x0"].shape),), run)


def test_postnet_training_step(S, dev, fresh):
    """The smallest fixture of tests/test_gpu_postnet_training.py: dim 128, B = 2, T = 48 with a ragged second sample."""
    PN, TO = _mod(".diffvc.model.postnet"), _mod(".model._train_ops")
    sd = PO.make_state(128, seed=5)
    g = torch.Generator().manual_seed(9)
    mask = torch.ones(2, 1, 48)
    mask[1, :, 37:] = 0
    z, gout = torch.randn(2, 80, 48, generator=g), torch.randn(2, 80, 48, generator=g)

    def run():
        pn = PN.PostNet(128)
        pn.load_state_dict(sd, strict=True)
        pn = pn.to(dev)
        zg = z.to(dev).requires_grad_()
        TO.reset_op_counts()
        out = pn(zg, mask.to(dev))
        (out * gout.to(dev)).sum().backward()
        assert TO.op_counts()[1] == 0 and TO.op_counts()[0] >= 7, TO.op_counts()
        return dict(_param_grads(pn), out=out.detach(), dz=zg.grad)

    fresh("PostNet training step", "dim 128 B 2 T 48 lengths (48, 37)", run)


@pytest.mark.parametrize("name,dropout", [("TextEncoder", False), ("Encoder", True), ("MelEncoder", True)])
def test_encoder_training_paths(dev, fresh, monkeypatch, name, dropout):
    """Both encoders' training paths -- attention, LayerNorm and Conv1d forward and backward -- at the module fixtures of
    tests/test_gpu_enc_train_modules.py and tests/test_gpu_enc_conv_train_modules.py (lengths (17, 9, 1)): the text encoder in eval(),
    the two Encoder stacks in train() with p_dropout 0.1 under the seed those suites draw their masks from."""
    import test_gpu_enc_conv_train_modules as EC
    M = type("M", (), {})()
    M.TE, M.ME, M.TO = _mod(".model.text_encoder"), _mod(".diffvc.model.encoder"), _mod(".model._train_ops")
    monkeypatch.setattr(M.TO, "ENC_CONV_KERNEL_FORWARD", True)
    monkeypatch.setattr(M.TO, "ENC_CONV_LEFT_ON_TORCH", frozenset())
    Lx = max(EC.LENS)
    g = torch.Generator().manual_seed(4)
    inputs = {"Encoder": lambda: (torch.randn(3, 24, Lx, generator=g), EC.seq_mask(EC.LENS, Lx)),
              "MelEncoder": lambda: (torch.randn(3, 8, Lx, generator=g), EC.seq_mask(EC.LENS, Lx)),
              "TextEncoder": lambda: (torch.randint(0, 30, (3, Lx), generator=g), torch.tensor(EC.LENS))}[name]()

    def build():
        torch.manual_seed(21)
        p = 0.1 if dropout else 0.0
        if name == "Encoder":
            return M.TE.Encoder(24, 48, n_heads=2, n_layers=2, kernel_size=3, p_dropout=p, window_size=4)
        if name == "MelEncoder":
            return M.ME.MelEncoder(8, 24, 48, 2, 2, 3, p, window_size=4)
        return M.TE.TextEncoder(30, 8, 24, 48, 16, 2, 2, 3, p, window_size=4)

    def run():
        mod = EC._randomise(build(), 6).to(dev)
        mod = mod.train() if dropout else mod.eval()
        M.TO.reset_enc_op_counts(), M.TO.reset_enc_conv_op_counts()
        torch.manual_seed(1234)
        call = (lambda m, i, n: m(i, n)[:2]) if name == "TextEncoder" else (lambda m, x, mk: m(x, mk))
        outs, grads = EC._grads(mod, call, EC._to(inputs, dev))
        assert M.TO.enc_op_counts()[0] > 0 and M.TO.enc_op_counts()[1] == 0                                             # on the kernels
        assert M.TO.enc_conv_op_counts() == (EC.n_convs(mod), 0), M.TO.enc_conv_op_counts()
        return dict({"d " + n: v for n, v in grads.items()}, **{"out%d" % k: o.detach() for k, o in enumerate(outs)})

    fresh("%s training path%s" % (name, " (dropout)" if dropout else ""), "B 3 L %d lengths %s" % (Lx, EC.LENS), run)


@pytest.mark.parametrize("N,T", [(17, 160), (2, 129)])
def test_speaker_encoder_training(S, dev, fresh, N, T):
    """forward_train + backward: (17, 160), and (2, 129), which gives two weight-gradient slices with a ragged last one."""
    sd = SO.state("default")
    x, up = SO.frames("noise", N, T), GO.upstream(N)

    def run():
        plan = S.SpkPlan()
        blob, blob_train = plan.pack(sd, dev), plan.pack_train(sd, dev)
        embeds, saved = plan.forward_train(blob, x.to(dev))
        grads = plan.backward(blob_train, x.to(dev), up.to(dev), saved)
        return dict({"d " + n: g for (n, _), g in zip(plan.param_layout(), grads)}, embeds=embeds)

    fresh("SpkPlan forward_train + backward", (N, T), run)


@pytest.mark.parametrize("S_,U", GO.GE2E_SHAPES[:2])
def test_ge2e_loss(S, dev, fresh, S_, U):
    e = GO.embeddings("model", S_, U)

    def run():
        sim, loss, d_embeds, dw, db = S.ge2e_loss(e.to(dev), torch.tensor([GO.W0], device=dev), torch.tensor([GO.B0], device=dev))
        return dict(sim=sim, loss=loss, d_embeds=d_embeds, dw=dw, db=db)

    fresh("ge2e_loss", "%d speakers x %d utterances" % (S_, U), run)


def test_mel_loss_backward_through_the_drop_in(dev, fresh):
    """hifi_gan.meldataset.mel_spectrogram under autograd, with lengths: the mel and the waveform's gradient."""
    MD = _mod(".hifi_gan.meldataset")
    Lw, lens = 256 * 19, [256 * 19, 845, 385]
    y = MO.signal("noise", Lw)[:3]
    dmel = torch.randn(3, 80, 19, generator=torch.Generator().manual_seed(20))

    def run():
        yd = y.to(dev).requires_grad_()
        mel, mel_lengths = MD.mel_spectrogram(yd, *MO.CFG1, y_lengths=lens)
        (mel * dmel.to(dev)).sum().backward()
        return dict(mel=mel.detach(), dwav=yd.grad, mel_lengths=mel_lengths)

    fresh("mel_spectrogram + backward (drop-in)", "cfg1 B 3 L %d lengths %s" % (Lw, tuple(lens)), run)
