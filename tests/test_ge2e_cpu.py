"""CPU: the speaker encoder's training side without a device -- the float64 checker (tests/ge2e_oracle.py) and the torch path of
diffvc/speaker_encoder/encoder/ge2e.py against what the reference's own SpeakerEncoder.loss recorded (tests/golden/ge2e.npz, written by
tests/golden/make_golden_ge2e.py), the EER recipe, the module's state_dict and do_gradient_ops, one whole step on CPU tensors, the
host-only refusals of the new entry points, and the fixture conditions the GPU tests (tests/test_gpu_spk_train.py) rest on.

Bounds against the golden: sim 5e-6 (float32 rounding of values in [-5, 5]), loss 2e-6, gradients 1e-5 of the tensor's largest entry.
similarity_bias.grad is analytically zero (each softmax row sums to one), so it is checked as |db| <= 1e-5 and never normalised."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import ge2e_oracle as GO
import spk_oracle as SO
from conftest import golden, pkg

GOLDEN_SHAPES = [(2, 2), (3, 4), (8, 5)]


@pytest.fixture(scope="module")
def G():
    return importlib.import_module("speech-backbones_amd.diffvc.speaker_encoder.encoder.ge2e")


@pytest.fixture(scope="module")
def gold():
    return golden("ge2e.npz")


def _gold(gold, kind, S, U):
    return {k: gold["%s_%d_%d_%s" % (kind, S, U, k)] for k in ("sim", "loss", "eer", "d_embeds", "dw", "db", "checksum")}


def _scalar(v):
    return float(np.asarray(v).reshape(-1)[0])


def _check(got, want):
    assert float(np.abs(got["sim"] - want["sim"]).max()) <= 5e-6
    assert abs(_scalar(got["loss"]) - _scalar(want["loss"])) <= 2e-6
    assert GO.err(got["d_embeds"], want["d_embeds"]) <= 1e-5
    assert GO.err(got["dw"], want["dw"]) <= 1e-5
    assert abs(_scalar(got["db"])) <= 1e-5 and abs(_scalar(want["db"])) <= 1e-5


@pytest.mark.parametrize("S,U", GOLDEN_SHAPES)
@pytest.mark.parametrize("kind", GO.KINDS)
def test_the_float64_oracle_reproduces_the_reference(gold, kind, S, U):
    want = _gold(gold, kind, S, U)
    assert abs(GO.checksum(GO.embeddings(kind, S, U)) - float(want["checksum"])) <= 1e-9        # the recorded input, regenerated
    g64, _ = GO.ge2e_reference(kind, S, U)
    _check({k: v.numpy() for k, v in g64.items()}, want)


@pytest.mark.parametrize("S,U", GOLDEN_SHAPES)
@pytest.mark.parametrize("kind", GO.KINDS)
def test_the_torch_path_of_the_module_reproduces_the_reference(G, gold, kind, S, U):
    want = _gold(gold, kind, S, U)
    m = G.SpeakerEncoder("cpu", "cpu")
    e = GO.embeddings(kind, S, U).clone().requires_grad_(True)
    loss, eer = m.loss(e)
    loss.backward()
    with torch.no_grad():
        sim = m.similarity_matrix(e)
    assert tuple(sim.shape) == (S, U, S) and loss.dim() == 0
    _check(dict(sim=sim.reshape(S * U, S).numpy(), loss=loss.item(), d_embeds=e.grad.numpy(), dw=m.similarity_weight.grad.numpy(),
                db=m.similarity_bias.grad.numpy()), want)
    assert abs(eer - float(want["eer"])) <= 1e-6            # (from this path's own float32 sim; the recorded sim: next test)
    loss2, none = m.loss(e.detach(), want_eer=False)
    assert none is None and float(loss2) == float(loss)
    # float64 embeddings take the same path
    assert m.loss(e.detach().double(), want_eer=False)[0].dtype == torch.float64


@pytest.mark.parametrize("S,U", GOLDEN_SHAPES)
@pytest.mark.parametrize("kind", GO.KINDS)
def test_eer_of_the_recorded_similarity_matrix(G, gold, kind, S, U):
    want = _gold(gold, kind, S, U)
    assert abs(G.equal_error_rate(want["sim"], U) - float(want["eer"])) <= 1e-9


def test_one_utterance_per_speaker_is_nan_as_in_the_reference(G):
    m = G.SpeakerEncoder("cpu", "cpu")
    e = GO.embeddings("model", 3, 4)[:, :1]
    assert bool(torch.isnan(m.loss(e, want_eer=False)[0]))
    assert bool(torch.isnan(GO.ge2e(e, GO.W0, GO.B0, torch.float64)["loss"]).all())


def test_state_dict_is_the_inference_class_and_its_checkpoints_load(G):
    parent = SO.encoder_pkg().SpeakerEncoder("cpu", "cpu")
    m = G.SpeakerEncoder("cpu", "cpu")
    assert issubclass(G.SpeakerEncoder, type(parent)) and G.SpeakerEncoder.__name__ == "SpeakerEncoder"
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in parent.state_dict().items()]
    assert m.load_state_dict(parent.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), parent.state_dict().values()))
    assert parent.load_state_dict(m.state_dict(), strict=True)
    with pytest.raises(NotImplementedError, match="GE2E training"):        # the inference class stays what it was
        parent.loss(torch.zeros(2, 2, 256))


def test_do_gradient_ops_is_the_two_lines_of_the_reference(G):
    m = G.SpeakerEncoder("cpu", "cpu")
    g = torch.Generator().manual_seed(5)
    grads = {k: torch.randn(p.shape, generator=g) for k, p in m.named_parameters()}
    twin = [torch.nn.Parameter(p.detach().clone()) for p in m.parameters()]
    for (k, p), q in zip(m.named_parameters(), twin):
        p.grad = grads[k].clone()
        q.grad = grads[k].clone() * (0.01 if k.startswith("similarity_") else 1.0)
    torch.nn.utils.clip_grad_norm_(twin, 3, norm_type=2)
    m.do_gradient_ops()
    for p, q in zip(m.parameters(), twin):
        assert torch.equal(p.grad, q.grad)
    total = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters()))
    assert abs(float(total) - 3) <= 1e-4


def test_one_whole_step_on_cpu_tensors(G):
    S, U, T = 3, 4, 7
    m = G.SpeakerEncoder("cpu", "cpu")
    m.load_state_dict(dict(SO.state("trained"), similarity_weight=torch.tensor([GO.W0]), similarity_bias=torch.tensor([GO.B0])))
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    loss, eer = m.loss(m(SO.frames("noise", S * U, T)).view(S, U, -1))
    loss.backward()
    grads = {k: p.grad.clone() for k, p in m.named_parameters()}
    assert len(grads) == 16 and all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
    assert 0.0 <= eer <= 1.0
    g64, e32, _, loss64 = GO.step_reference(S, U, T)
    assert abs(float(loss) - float(loss64)) <= 2e-6
    for k, g in grads.items():
        if k == "similarity_bias":
            assert abs(float(g)) <= 1e-5
        else:
            assert GO.err(g, g64[k]) <= 4 * e32[k] + 2e-6, k
    m.do_gradient_ops()
    opt.step()


# ---- host-only refusals of the entry points of csrc/spk_train.hip: every call is made with addresses of nothing and must return before
# one of them is followed or a kernel is launched
E_NULL, E_SHAPE, E_PARAMS, E_WORKSPACE = -1, -2, -5, -6


def test_training_entry_points_refuse_on_the_host():
    S = pkg()
    L = S._lib.lib()
    plan = S.SpkPlan()
    fake = ctypes.c_void_p(4096)
    big = 1 << 40
    # sizes: exact at the training shape, monotone across the tile, zero for what is refused
    assert plan.saved_bytes(640, 160) == 1888747520
    assert plan.saved_bytes(17, 160) > plan.saved_bytes(16, 160) and plan.train_workspace_bytes(17, 160) > plan.train_workspace_bytes(16, 160)
    assert L.gtts_spktrain_packed_bytes(plan._h) >= (3 + 2) * 1024 * 256 * 4 + 256 * 256 * 4
    for N, T in ((0, 160), (-1, 160), (4, 0), (4, -3), (1 << 14, 160)):                      # 2^14 * 160 * 1024 >= 2^31
        assert plan.saved_bytes(N, T) == 0 and plan.train_workspace_bytes(N, T) == 0
    assert L.gtts_spktrain_packed_bytes(None) == 0 and L.gtts_spktrain_saved_bytes(None, 4, 160) == 0
    assert L.gtts_spktrain_workspace_bytes(None, 4, 160) == 0
    # forward
    fwd = lambda N, T, nbytes=big, h=plan._h, blob=fake, x=fake, e=fake, sv=fake: L.gtts_spktrain_forward(h, blob, x, N, T, e, sv, nbytes, None)
    for N, T in ((0, 160), (-1, 160), (4, 0), (4, -3), (1 << 14, 160)):
        assert fwd(N, T) == E_SHAPE
    assert fwd(4, 160, plan.saved_bytes(4, 160) - 1) == E_WORKSPACE and b"too small" in L.gtts_last_error()
    assert fwd(4, 160, 0) == E_WORKSPACE
    for kw in (dict(h=None), dict(blob=None), dict(x=None), dict(e=None), dict(sv=None)):
        assert fwd(4, 160, **kw) == E_NULL
    # backward
    grads = (ctypes.c_void_p * 14)(*([4096] * 14))

    def bwd(N, T, saved_bytes=big, ws_bytes=big, n=14, g=grads, **null):
        a = dict(h=plan._h, blob=fake, x=fake, d=fake, sv=fake, ws=fake)
        a.update(null)
        return L.gtts_spktrain_backward(a["h"], a["blob"], a["x"], a["d"], a["sv"], saved_bytes, g, n, a["ws"], ws_bytes, N, T, None)
    for N, T in ((0, 160), (-1, 160), (4, 0), (4, -3), (1 << 14, 160)):
        assert bwd(N, T) == E_SHAPE
    assert bwd(4, 160, saved_bytes=plan.saved_bytes(4, 160) - 1) == E_WORKSPACE
    assert bwd(4, 160, ws_bytes=plan.train_workspace_bytes(4, 160) - 1) == E_WORKSPACE and b"workspace too small" in L.gtts_last_error()
    for k in ("h", "blob", "x", "d", "sv", "ws"):
        assert bwd(4, 160, **{k: None}) == E_NULL, k
    assert bwd(4, 160, g=None) == E_NULL
    assert bwd(4, 160, n=13) == E_PARAMS and b"expected 14" in L.gtts_last_error()
    holed = (ctypes.c_void_p * 14)(*([4096] * 13 + [None]))
    assert bwd(4, 160, g=holed) == E_NULL and b"linear.bias" in L.gtts_last_error()
    # pack
    arr = (ctypes.c_void_p * 13)(*([4096] * 13))
    assert L.gtts_spktrain_pack(plan._h, arr, 13, fake, None) == E_PARAMS
    assert L.gtts_spktrain_pack(plan._h, None, 14, fake, None) == E_NULL and L.gtts_spktrain_pack(plan._h, grads, 14, None, None) == E_NULL
    with pytest.raises(RuntimeError, match="HIP device"):
        plan.forward_train(None, torch.zeros(1, 160, 40))


def test_ge2e_entry_point_refuses_on_the_host():
    S = pkg()
    L = S._lib.lib()
    fake = ctypes.c_void_p(4096)
    big = 1 << 40

    def loss(S_, U, E, nbytes=big, **null):
        a = dict(e=fake, w=fake, b=fake, sim=fake, loss=fake, de=fake, dw=fake, db=fake, ws=fake)
        a.update(null)
        return L.gtts_ge2e_loss(a["e"], a["w"], a["b"], S_, U, E, a["sim"], a["loss"], a["de"], a["dw"], a["db"], a["ws"], nbytes, None)
    for shape in ((0, 10, 256), (64, 0, 256), (64, 10, 0), (-1, 10, 256), (1025, 10, 256), (1024, 1 << 12, 1024)):
        assert loss(*shape) == E_SHAPE, shape
        assert L.gtts_ge2e_workspace_bytes(*shape) == 0
    need = L.gtts_ge2e_workspace_bytes(64, 10, 256)
    assert need >= (640 * 64 + 640 * 256 + 4 * 64 * 256) * 4
    assert loss(64, 10, 256, need - 1) == E_WORKSPACE and loss(64, 10, 256, 0) == E_WORKSPACE
    for k in ("e", "w", "b", "sim", "loss", "ws"):
        assert loss(64, 10, 256, **{k: None}) == E_NULL, k
    # the gradient outputs are optional: a call without them gets past the pointer checks and stops at the workspace
    assert loss(64, 10, 256, 0, de=None, dw=None, db=None) == E_WORKSPACE
    with pytest.raises(RuntimeError, match="HIP device"):
        S.ge2e_loss(torch.zeros(2, 2, 256), torch.ones(1), torch.ones(1))


# ---- what the GPU tests rest on, for every one of their cases
@pytest.mark.parametrize("N,T", GO.ENC_SHAPES)
@pytest.mark.parametrize("inputs", SO.INPUTS)
@pytest.mark.parametrize("weights", SO.WEIGHTS)
def test_fixture_conditions_of_the_encoder_cases(weights, inputs, N, T):
    g64, e32, pre64 = GO.encoder_reference(weights, inputs, N, T)
    assert int(GO.near_zero(pre64).sum()) <= 8
    assert set(g64) == set(GO.PARAMS) and max(e32.values()) <= 2.5e-4, e32
    if T == 1:
        assert all(float(g64["lstm.weight_hh_l%d" % l].abs().max()) == 0.0 for l in range(3))


@pytest.mark.parametrize("S,U,T", GO.STEP_SHAPES)
def test_fixture_conditions_of_the_step_cases(S, U, T):
    g64, e32, pre64, _ = GO.step_reference(S, U, T)
    assert int(GO.near_zero(pre64).sum()) <= 8
    assert len(g64) == 16 and max(e32.values()) <= 2.5e-4, e32


@pytest.mark.parametrize("S,U", GO.GE2E_SHAPES)
@pytest.mark.parametrize("kind", GO.KINDS)
def test_fixture_conditions_of_the_loss_cases(kind, S, U):
    g64, e32 = GO.ge2e_reference(kind, S, U)
    assert max(e32.values()) <= 2.5e-4 and abs(float(g64["db"])) <= 1e-12
