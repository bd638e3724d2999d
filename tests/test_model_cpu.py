"""CPU: host-side mirror of the reference interface (state_dict layout, parameter counts, helper functions,
training composition) and the rule that sampling never silently falls back to CPU."""
import importlib

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import gradtts_oracle as O

ARGS = (149, 1, 64, 192, 768, 256, 2, 6, 3, 0.1, 4, 80, 64, 0.05, 20.0, 1000)


@pytest.fixture(scope="module")
def M():
    return importlib.import_module("speech-backbones_amd.model")


def test_parameter_counts_match_survey(M):
    m = M.GradTTS(*ARGS)
    assert m.nparams == 14835032 and m.decoder.nparams == 7634887 and m.encoder.nparams == 7200145
    m2 = M.GradTTS(149, 247, *ARGS[2:])
    assert m2.nparams == 14888680 and m2.decoder.nparams == 7672727
    assert tuple(m2.spk_emb.weight.shape) == (247, 64)


def test_decoder_state_dict_equals_oracle_layout(M):
    D = importlib.import_module("speech-backbones_amd.model.diffusion")
    for n_spks in (1, 4):
        dec = D.Diffusion(80, 64, n_spks, 64, 0.05, 20.0, 1000)
        got = [(k, tuple(v.shape)) for k, v in dec.state_dict().items()]
        want = [("estimator." + k, tuple(v.shape)) for k, v in O.make_estimator_state(n_spks=n_spks).items()]
        assert got == want


def test_utils_match_reference_golden(M):
    U = importlib.import_module("speech-backbones_amd.model.utils")
    g = golden("utils.npz")
    t = lambda a: torch.from_numpy(np.asarray(a))
    assert np.array_equal(U.sequence_mask(t(g["lens"]), 9).numpy(), g["seqmask"])
    assert [U.fix_len_compatibility(n) for n in range(20)] == list(g["fixlen"])
    assert np.array_equal(U.generate_path(t(g["dur"]), t(g["pmask"])).numpy(), g["path"])
    assert U.convert_pad_shape([[0, 0], [1, 0], [0, 0]]) == [0, 0, 1, 0, 0, 0]


def test_training_composition_matches_oracle_and_has_gradients(M):
    D = importlib.import_module("speech-backbones_amd.model.diffusion")
    sd = O.make_estimator_state(seed=5)
    dec = D.Diffusion(80, 64, 1, 64, 0.05, 20.0, 1000)
    dec.estimator.load_state_dict(sd, strict=True)
    inp = O.make_inputs(2, 32)
    t = torch.tensor([0.3, 0.8])
    est = dec.estimator(inp["z"], inp["mask"], inp["mu"], t)           # autograd enabled -> torch composition
    assert torch.allclose(est, O.estimator_forward(sd, inp["z"], inp["mask"], inp["mu"], t), atol=1e-5)
    torch.manual_seed(0)
    loss, xt = dec.compute_loss(inp["z"], inp["mask"], inp["mu"])
    loss.backward()
    assert torch.isfinite(loss) and dec.estimator.final_conv.weight.grad is not None


def test_sampling_on_cpu_raises_instead_of_falling_back(M):
    D = importlib.import_module("speech-backbones_amd.model.diffusion")
    dec = D.Diffusion(80, 64, 1, 64, 0.05, 20.0, 1000)
    inp = O.make_inputs(1, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec(inp["z"], inp["mask"], inp["mu"], 2)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        dec.estimator(inp["z"], inp["mask"], inp["mu"], torch.ones(1))
    # MAS is the exception the reference itself makes: its wrapper takes tensors on any device and runs the host kernel
    # (monotonic_align/__init__.py:8-23); host tensors go to the library's C++ twin, not to a PyTorch fallback
    MA = importlib.import_module("speech-backbones_amd.model.monotonic_align")
    p = MA.maximum_path(torch.zeros(1, 3, 5), torch.ones(1, 3, 5))
    assert p.shape == (1, 3, 5) and float(p.sum()) == 5.0


def test_pack_spec_list_lives_and_dies_with_the_estimator(M):
    """The batched-pack plan of the training path hangs off the spec list, the list off the estimator (no module-global table): a
    replaced Parameter rebuilds the list, a deleted estimator frees it (and with it the packed blobs the plan would hold)."""
    import gc
    import weakref
    D = importlib.import_module("speech-backbones_amd.model.diffusion")
    T = importlib.import_module("speech-backbones_amd.model._train_ops")
    dec = D.Diffusion(80, 64, 1, 64, 0.05, 20.0, 1000)
    est = dec.estimator
    specs = T._pack_specs(est)
    assert isinstance(specs, T.backend().PackSpecs) and len(specs) >= 2 * 24 and len(specs.mods) == len(specs)
    assert T._pack_specs(est) is specs
    conv = est.mid_block1.block1.block[0]
    old = conv.weight
    conv.weight = torch.nn.Parameter(old.detach().clone())
    again = T._pack_specs(est)
    assert again is not specs and all(s[0] is not old for s in again) and any(s[0] is conv.weight for s in again)
    assert not hasattr(T.backend(), "_PACK_PLANS")
    ref = weakref.ref(again)
    del dec, est, specs, again, conv, old
    gc.collect()
    assert ref() is None


def test_plan_variant_by_batch_size(M):
    """The drop-in estimator picks its plan by batch size in the default precision (model/diffusion.py::_variant): the persistent kernel,
    unsplit, at B = 1 and B >= 7; the uniform-wave kernel on three sub-batch streams for B = 2..6; one plan per variant, rebuilt by
    set_precision; the other precisions keep a single plan."""
    D = importlib.import_module("speech-backbones_amd.model.diffusion")
    S = importlib.import_module("speech-backbones_amd")
    est = D.Diffusion(80, 64, 1, 64, 0.05, 20.0, 1000).estimator
    assert [est._variant(b) for b in (None, 1, 2, 6, 7, 16, 32)] == ["main", "main", "mid", "mid", "main", "main", "main"]
    p1, p4, p16 = est._plan(1), est._plan(4), est._plan(16)
    assert p1 is p16 and p4 is not p1 and est._plan(6) is p4
    assert p1.conv_ws is True and p1._nstreams == 0 and p1.cfg.precision == S.PREC_F16F8
    assert p4.conv_ws is False and p4._nstreams == 3 and p4.cfg.precision == S.PREC_F16F8
    est.set_precision("bf16x3")
    assert [est._variant(b) for b in (1, 4, 16)] == ["main"] * 3
    q = est._plan(4)
    assert q is not p4 and q is est._plan(16) and q.cfg.precision == S.PREC_BF16X3
    with pytest.raises(KeyError):
        est.set_precision("fp64")


def test_drop_in_as_top_level_model_package():
    """`PYTHONPATH=speech-backbones_amd python -c 'from model import GradTTS'` -- how inference.py imports it."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    code = ("from model import GradTTS; from model.utils import fix_len_compatibility; import model.monotonic_align as m;"
            "g = GradTTS(149,1,64,192,768,256,2,6,3,0.1,4,80,64,0.05,20.0,1000); print(g.nparams, fix_len_compatibility(171))")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "speech-backbones_amd"))
    out = subprocess.check_output([sys.executable, "-c", code], env=env, cwd="/tmp").decode().split()
    assert out == ["14835032", "172"]


def test_whole_model_against_reference_live(M):
    """Against the reference's GradTTS (its layout, encoder outputs and losses in tests/golden/live_gradtts.npz, make_golden_live.py): under
    torch.manual_seed(0) the drop-in model must reproduce the reference's default initialisation, which those were computed with."""
    from live_golden import assert_reference_init, live
    G = live()
    torch.manual_seed(0)
    m = M.GradTTS(*ARGS).eval()
    assert_reference_init(m.state_dict(), G, "gradtts")
    x = torch.from_numpy(G["gradtts_x"])
    xl = torch.tensor([37, 21])
    with torch.no_grad():
        for i, b in enumerate(m.encoder(x, xl)):
            assert torch.allclose(torch.from_numpy(G["gradtts_enc%d" % i]), b, atol=1e-5)
    # compute_loss host logic end to end, MAS through the library's own host twin (gtts_mas_maximum_path_cpu): without
    # and with the random training crop (same `random` / torch RNG streams -> same windows, same noise)
    import random
    y = torch.from_numpy(G["gradtts_y"])
    yl = torch.tensor([60, 44])
    for out_size in (None, 48, 52):
        random.seed(5)
        torch.manual_seed(1)
        lb = m.compute_loss(x, xl, y, yl, out_size=out_size)
        for i, b in enumerate(lb):
            assert torch.allclose(torch.from_numpy(G["gradtts_loss_%s_%d" % (out_size, i)]), b, rtol=1e-4, atol=1e-5), out_size


@pytest.mark.parametrize("n_spks", [1, 3])
def test_parameter_gradients_match_reference_loss_t(n_spks):
    """Every parameter's gradient of the product's CPU composition against the REFERENCE module's `Diffusion.loss_t`
    (Grad-TTS/model/diffusion.py:281-288) on the same weights, inputs, t and noise draw.  This is the reference pin the GPU
    gradient test (tests/test_gpu_training.py: HIP kernels vs this CPU composition) inherits.  The reference's loss, noised
    sample and, per parameter, gradient norm, max |.| and 64 entries are stored in tests/golden/live_grads.npz."""
    from live_golden import GOLDEN_THREADS, live, sample_index
    G = live()
    threads = torch.get_num_threads()
    torch.set_num_threads(GOLDEN_THREADS)          # the stored gradients' thread count (their last bits depend on it)
    try:
        _check_gradients_against_golden(G, n_spks, sample_index)
    finally:
        torch.set_num_threads(threads)


def _check_gradients_against_golden(G, n_spks, sample_index):
    tag = "grad_s%d" % n_spks
    D = importlib.import_module("speech-backbones_amd.model.diffusion")
    sd = O.make_estimator_state(n_spks=n_spks, seed=11)
    spk_dim = 64
    own = D.Diffusion(80, 64, n_spks, spk_dim, 0.05, 20.0, 1000)
    own.estimator.load_state_dict(sd, strict=True)
    inp = O.make_inputs(2, 36, seed=2, spk_dim=spk_dim if n_spks > 1 else None)
    t = torch.tensor([0.35, 0.8])
    spk = inp.get("spk")
    la, xta = torch.from_numpy(G[tag + "_loss"]), torch.from_numpy(G[tag + "_xt"])
    torch.manual_seed(4)
    lb, xtb = own.loss_t(inp["z"], inp["mask"], inp["mu"], t, spk)
    assert float((xta - xtb).abs().max()) <= 1e-5          # elementwise ops: bit-identical live, last bits across CPUs
    assert torch.allclose(la, lb, rtol=1e-5, atol=1e-7)
    lb.backward()
    has = dict(zip((str(k) for k in G[tag + "_names"]), G[tag + "_has_grad"]))
    assert sorted(has) == sorted(n for n, _ in own.estimator.named_parameters())
    n, off = 0, 0
    for name, p in own.estimator.named_parameters():
        assert (p.grad is None) == (not has[name]), name
        if p.grad is None:
            continue
        g = p.grad.detach().double().flatten().numpy()
        idx = sample_index(g.size)
        want = G[tag + "_vals"][off:off + idx.size]
        off += idx.size
        scale = float(G[tag + "_max"][n]) + 1e-12
        assert abs(float(np.sqrt((g * g).sum())) - float(G[tag + "_norm"][n])) <= 2e-5 * float(G[tag + "_norm"][n]) + 1e-9, name
        assert float(np.abs(g[idx] - want).max()) <= 2e-5 * scale + 1e-9, (name, float(np.abs(g[idx] - want).max()), scale)
        n += 1
    assert n >= 172


@pytest.mark.parametrize("tag,n_spks", [("s1", 1), ("s3", 3)])
def test_loss_and_gradients_match_reference_golden(tag, n_spks):
    """The same comparison without /root/reference (what travels to the GPU box): tests/golden/loss_grads.npz holds the
    reference's loss, noised sample and, per parameter, gradient norm / max / 16 entries (make_golden_grads.py)."""
    import numpy as np
    import os
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_grads.npz"))
    D = importlib.import_module("speech-backbones_amd.model.diffusion")
    sd = O.make_estimator_state(n_spks=n_spks, seed=int(G[tag + "_seed"]))
    assert abs(sum(float(v.double().abs().sum()) for v in sd.values()) - float(G[tag + "_checksum"])) <= 1e-6 * float(G[tag + "_checksum"])
    dec = D.Diffusion(80, 64, n_spks, 64, 0.05, 20.0, 1000)
    dec.estimator.load_state_dict(sd, strict=True)
    from helpers_golden import check_against_golden_grads
    check_against_golden_grads(dec, G, tag, torch.device("cpu"), 2e-5)
