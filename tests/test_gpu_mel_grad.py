"""GPU tests (-m gpu) of the log-mel input gradient (csrc/mel_train.hip) through the C ABI, MelPlan.backward and the drop-in
hifi_gan/meldataset.py under autograd, against float64 autograd through the recipe on the CPU (tests/mel_grad_cases.py, whose CPU
test proves the yardstick: the hand-written float64 backward equals autograd, every restated mistake exceeds the bound used here).

Error of a row: max-abs over the row's max |ref|.  Bound: e <= 4 e_ref32 + 2e-6 (e_ref32: the recipe under float32 autograd on the
CPU) on noise, quiet, impulse and the half-clipped signal; exactly 0 on zeros; on speechlike, whose gradient is ill-conditioned, the
ratio is printed and the mistake-separating bound mel_grad_cases.SPEECH_BOUND is asserted.  With -s every parity case prints a row
(recorded in profiles/mel_grad_parity.txt).  dwav and the workspace sit between NaN margins in every raw call."""
import ctypes
import importlib
import warnings

import pytest
import torch
import torch.nn.functional as F

import mel_grad_cases as C
import mel_oracle as MO
from gpu_guards import S, dev  # noqa: F401
from oracle import hifigan_oracle as H

pytestmark = pytest.mark.gpu
MARGIN = 4096                                            # floats of NaN on both sides of dwav, bytes of 0xff around the workspace
PARITY = [(c, B) for c in C.CASES for B in ((3,) if c[2] else (1, 2, 3))]          # (the ragged case is its three rows)


@pytest.fixture(scope="module")
def MD():
    return importlib.import_module("speech-backbones_amd.hifi_gan.meldataset")


@pytest.fixture(scope="module")
def plans(S, dev):
    made = {}

    def get(cfg):
        if cfg not in made:
            plan = S.MelPlan(*cfg)
            made[cfg] = (plan, plan.pack(dev))
        return made[cfg]
    return get


@pytest.fixture(scope="module")
def raw(S, plans, dev):
    """raw(cfg, y, dmel, lengths=None) -> dwav on the CPU: gtts_mel_backward itself, dwav and the workspace between margins that must
    come back untouched."""
    def go(cfg, y, dmel, lengths=None):
        plan, blob = plans(cfg)
        B, L = y.shape
        yd, dd = y.to(dev).contiguous(), dmel.to(dev).contiguous()
        ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
        need = plan.backward_workspace_bytes(B, L)
        out = torch.full((B * L + 2 * MARGIN,), float("nan"), dtype=torch.float32, device=dev)
        ws = torch.full((need + 2 * MARGIN,), 0xff, dtype=torch.uint8, device=dev)
        ptr = lambda t, off=0: ctypes.c_void_p(0 if t is None else t.data_ptr() + off)
        rc = S._lib.lib().gtts_mel_backward(plan._h, ptr(blob), ptr(yd), ptr(ld), ptr(dd), ptr(out, 4 * MARGIN), ptr(ws, MARGIN), need, B, L,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, S._lib.lib().gtts_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[:MARGIN]).all()) and bool(torch.isnan(out[-MARGIN:]).all())
        assert bool((ws[:MARGIN] == 0xff).all()) and bool((ws[-MARGIN:] == 0xff).all())
        return out[MARGIN:-MARGIN].view(B, L).cpu()
    return go


@pytest.mark.parametrize("case,B", PARITY, ids=["%s-B%d" % (C.case_id(c), B) for c, B in PARITY])
def test_parity_with_float64_autograd(raw, case, B):
    tag, L, lens, name = case
    cfg, r = C.CFGS[tag], C.reference(case)
    got = raw(cfg, r["y"][:B], r["dmel"][:B], list(lens) if lens else None)
    assert got.shape == (B, L) and bool(torch.isfinite(got).all())
    e, e32 = C.row_error(got, r["ref"][:B]), r["e_ref32"][:B]
    worst = max(range(B), key=lambda b: float(e[b]) / C.gpu_bound(case, e32[b]))
    print("\n%-40s B=%d e %.2e  e_ref32 %.2e  ratio %.2f  clipped %.3f" % (C.case_id(case), B, float(e[worst]), float(e32[worst]),
                                                                         float(e[worst]) / max(float(e32[worst]), 1e-30), r["clipped"]))
    if name == "zeros":
        assert bool((got == 0).all())
    for b in range(B):
        assert float(e[b]) <= C.gpu_bound(case, e32[b])
    if lens:
        for b, n in C.rows_of(case):
            assert bool((got[b, n:] == 0).all())


def test_binding_equals_the_raw_call(raw, plans, dev):
    case = ("cfg1", C.L37, None, "noise")
    r = C.reference(case)
    plan, blob = plans(MO.CFG1)
    got = plan.backward(blob, r["y"].to(dev), r["dmel"].to(dev))
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), raw(MO.CFG1, r["y"], r["dmel"]))
    with pytest.raises(RuntimeError, match="dmel must be"):
        plan.backward(blob, r["y"].to(dev), r["dmel"][:, :, :-1].to(dev))
    with pytest.raises(RuntimeError, match="lengths"):
        plan.backward(blob, r["y"].to(dev), r["dmel"].to(dev), torch.tensor([C.L37, 845, 385]))


@pytest.mark.parametrize("case", [("cfg1", C.L37, None, "speechlike"), ("cfg1", 845, None, "halfclip"), ("cfg2", 160 * 59 + 31, None, "noise"),
                                  ("n2048-full", 512 * 19 + 77, None, "noise")], ids=C.case_id)
def test_determinism_batch_independence_and_scaling(raw, case):
    cfg, r = C.CFGS[case[0]], C.reference(case)
    a = raw(cfg, r["y"], r["dmel"])
    assert torch.equal(a, raw(cfg, r["y"], r["dmel"]))                      # no floating-point atomics: the same bits
    for b in range(MO.ROWS):
        assert torch.equal(a[b:b + 1], raw(cfg, r["y"][b:b + 1], r["dmel"][b:b + 1]))
    assert torch.equal(raw(cfg, r["y"], 2 * r["dmel"]), 2 * a)              # linear in dmel, and a power of two is exact


def test_ragged_rows_equal_the_rows_run_alone(raw):
    case = (C.RAGGED[0], C.RAGGED[1], C.RAGGED[2], "speechlike")
    r = C.reference(case)
    got = raw(MO.CFG1, r["y"], r["dmel"], list(C.RAGGED[2]))
    for b, n in C.rows_of(case):
        Tb = MO.frames(MO.CFG1, n)
        alone = raw(MO.CFG1, r["y"][b:b + 1, :n], r["dmel"][b:b + 1, :, :Tb])
        assert torch.equal(got[b:b + 1, :n], alone) and bool((got[b, n:] == 0).all())


def test_drop_in_gives_the_generated_waveform_a_gradient(MD, plans, dev):
    case = ("cfg1", C.L37, None, "noise")
    r = C.reference(case)
    plan, blob = plans(MO.CFG1)
    yd, dd = r["y"].to(dev), r["dmel"].to(dev)
    want_mel, want_grad = MD.mel_spectrogram(yd, *MO.CFG1), plan.backward(blob, yd, dd)
    assert not want_mel.requires_grad
    y = yd.clone().requires_grad_()
    mel = MD.mel_spectrogram(y, *MO.CFG1)
    assert mel.requires_grad and mel.grad_fn is not None
    assert torch.equal(mel.detach(), want_mel)                              # the same launch: bit-equal to the no-grad path
    (mel * dd).sum().backward()
    assert torch.equal(y.grad, want_grad)
    with torch.no_grad():                                                   # grad mode off: today's path
        assert not MD.mel_spectrogram(y, *MO.CFG1).requires_grad
    # strided and float64 inputs get their gradient through torch's own conversion
    ys = yd.t().contiguous().t().requires_grad_()
    assert not ys.is_contiguous()
    mel = MD.mel_spectrogram(ys, *MO.CFG1)
    assert torch.equal(mel.detach(), want_mel)
    (mel * dd).sum().backward()
    assert ys.grad.shape == ys.shape and torch.equal(ys.grad, want_grad)
    y64 = yd.double().requires_grad_()
    mel = MD.mel_spectrogram(y64, *MO.CFG1)
    assert torch.equal(mel.detach(), want_mel)
    (mel * dd).sum().backward()
    assert y64.grad.dtype == torch.float64 and torch.equal(y64.grad, want_grad.double())
    # center=True keeps the torch recipe, differentiable as before
    yc = yd.clone().requires_grad_()
    MD.mel_spectrogram(yc, *MO.CFG1, center=True).sum().backward()
    assert bool(torch.isfinite(yc.grad).all()) and float(yc.grad.abs().max()) > 0


def test_drop_in_with_lengths(MD, plans, dev):
    case = (C.RAGGED[0], C.RAGGED[1], C.RAGGED[2], "noise")
    r = C.reference(case)
    plan, blob = plans(MO.CFG1)
    yd, dd, lens = r["y"].to(dev), r["dmel"].to(dev), list(C.RAGGED[2])
    for given in (lens, torch.tensor(lens, device=dev)):
        y = yd.clone().requires_grad_()
        mel, mel_lengths = MD.mel_spectrogram(y, *MO.CFG1, y_lengths=given)
        assert mel.grad_fn is not None and mel_lengths.tolist() == [37, 3, 1]
        assert torch.equal(mel.detach(), MD.mel_spectrogram(yd, *MO.CFG1, y_lengths=given)[0])
        (mel * dd).sum().backward()
        for b, n in C.rows_of(case):
            Tb = MO.frames(MO.CFG1, n)
            assert bool((y.grad[b, n:] == 0).all())
            assert torch.equal(y.grad[b:b + 1, :n], plan.backward(blob, yd[b:b + 1, :n], dd[b:b + 1, :, :Tb]))
        assert float(C.row_error(y.grad.cpu(), r["ref"]).max()) <= 4 * float(r["e_ref32"].max()) + 2e-6


def test_a_tensor_without_requires_grad_allocates_the_output_only(MD, dev):
    """Grad mode on, y does not require grad: the old path -- no workspace, nothing saved (the memory pattern of
    test_gpu_mel.py::test_one_call_allocates_the_output_only)."""
    y = MO.signal("noise", 256 * 130).to(dev)
    assert torch.is_grad_enabled()
    MD.mel_spectrogram(y, *MO.CFG1)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    out = MD.mel_spectrogram(y, *MO.CFG1)
    torch.cuda.synchronize()
    out_bytes = (out.numel() * 4 + 511) // 512 * 512
    assert out.grad_fn is None and tuple(out.shape) == (3, 80, 130)
    assert torch.cuda.memory_allocated(dev) - before == out_bytes
    assert torch.cuda.max_memory_allocated(dev) - before == out_bytes


def test_the_mel_loss_reaches_every_generator_parameter(MD, dev):
    """loss_mel of the HiFi-GAN training step on the smallest drop-in Generator in train(): every parameter gradient against the same
    module and recipe in float64 on the CPU, error over the tensor's largest element, bound 4 x the float32 CPU run's error + 2e-6.
    The L1 loss's sign makes cells with |mel - target| within 1e-4 ambiguous: the target is the mel of an unrelated signal, at most
    1 % of the cells fall in that band, and their weight is zero.  On a constant mel every one of these gradients is None or 0."""
    warnings.simplefilter("ignore")
    M = importlib.import_module("speech-backbones_amd.hifi_gan.models")
    env = importlib.import_module("speech-backbones_amd.hifi_gan.env")
    cfg = H.SMALL
    h = env.AttrDict(dict(cfg, upsample_rates=list(cfg["upsample_rates"]), upsample_kernel_sizes=list(cfg["upsample_kernel_sizes"]),
                          resblock_kernel_sizes=list(cfg["resblock_kernel_sizes"]),
                          resblock_dilation_sizes=[list(d) for d in cfg["resblock_dilation_sizes"]]))

    def make(dtype, device):                           # (weight-normalised modules do not deepcopy: built again from the same seed)
        torch.manual_seed(1)
        return M.Generator(h).to(device=device, dtype=dtype).train()      # (as initialised: scaled up, its output tanh saturates and
                                                                            #  every gradient underflows to 0)
    T = 2                                              # 512 samples, two frames, both reflections: the bound's 2e-6 floor is two float32
                                                       # ulps of a sum of about a thousand terms, and torch's own convolution backward
                                                       # on the device sums B * 256 * T terms per weight in the last stage
    x = H.make_mel(2, T, seed=2)
    target = MO.recipe(MO.signal("noise", 256 * T)[:2], MO.CFG1)             # float64 mel of an unrelated signal

    def grads(module, dtype, mel_fn, device):
        module.zero_grad()
        wav = module(x.to(device=device, dtype=dtype)).squeeze(1)
        mel = mel_fn(wav)
        w = wgt.to(device=device, dtype=mel.dtype)
        loss = F.l1_loss(w * target.to(device=device, dtype=mel.dtype), w * mel) * 45
        loss.backward()
        return {k: (None if p.grad is None else p.grad.detach().double().cpu()) for k, p in module.named_parameters()}, mel.detach().double().cpu()

    gen64 = make(torch.float64, "cpu")
    wgt = torch.ones_like(target)
    _, mel64 = grads(gen64, torch.float64, lambda w: MO.recipe(w, MO.CFG1), "cpu")
    band = (mel64 - target).abs() <= 1e-4
    assert float(band.double().mean()) <= 0.01
    assert float(mel64.min()) > -11.0                                       # no cell of the generated mel near the clip
    wgt = (~band).double()
    g64, _ = grads(gen64, torch.float64, lambda w: MO.recipe(w, MO.CFG1), "cpu")
    g32, _ = grads(make(torch.float32, "cpu"), torch.float32, lambda w: MO.recipe(w, MO.CFG1, torch.float32), "cpu")
    gdev, mel_dev = grads(make(torch.float32, dev), torch.float32, lambda w: MD.mel_spectrogram(w, *MO.CFG1), dev)
    assert float((mel_dev - mel64).abs().max()) <= 1e-3
    worst = 0.0
    for k, ref in g64.items():
        assert ref is not None and gdev[k] is not None and float(gdev[k].abs().max()) > 0, k
        scale = float(ref.abs().max())
        e_dev, e_32 = float((gdev[k] - ref).abs().max()) / scale, float((g32[k] - ref).abs().max()) / scale
        print("%-40s e %.2e  e_cpu32 %.2e  ratio %.2f" % (k, e_dev, e_32, e_dev / max(e_32, 1e-30)))
        worst = max(worst, e_dev / (4 * e_32 + 2e-6))
        assert e_dev <= 4 * e_32 + 2e-6, k
    print("worst e / bound %.2f" % worst)
