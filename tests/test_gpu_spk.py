"""GPU tests (-m gpu) of the speaker encoder kernels (csrc/spk.hip) through SpkPlan and the drop-in diffvc/speaker_encoder/encoder
against the float64 restatement on the CPU (tests/spk_oracle.py).

Bounds.  Parity: max |hidden - ref| <= 1e-3 and max |embeds - ref| <= 1e-3, the project's bound of record for fp32-grade paths, on the
O(1) hidden state and the unit-norm embedding.  Precision: the kernels are fp32 throughout (fp32-input MFMA = an fmaf chain, expf,
tanhf), so e_kernel <= 4 e_ref32 + 2e-6 is asserted as well, e_ref32 being the same recipe in float32 torch on the CPU; with -s every
case prints both and their ratio.  Batch and slicing independence: bit for bit.  The sequence tile is 16: (17, 160) crosses it."""

import numpy as np
import pytest
import torch

import spk_oracle as SO
from gpu_guards import S, dev  # noqa: F401

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 2), (3, 7), (16, 160), (17, 160), (1, 1000)]


@pytest.fixture(scope="module")
def run(S, dev):
    """run(weights, frames, **kw): SpkPlan.forward on CPU frames, plan and blob made once per weight kind; results on the CPU."""
    made = {}

    def go(weights, x, **kw):
        if weights not in made:
            plan = S.SpkPlan()
            made[weights] = (plan, plan.pack(SO.state(weights), dev))
        plan, blob = made[weights]
        out = plan.forward(blob, x.to(dev), **kw)
        return out.cpu() if torch.is_tensor(out) else tuple(o.cpu() for o in out)
    return go


@pytest.mark.parametrize("N,T", SHAPES)
@pytest.mark.parametrize("inputs", SO.INPUTS)
@pytest.mark.parametrize("weights", SO.WEIGHTS)
def test_parity_with_the_float64_recipe(run, weights, inputs, N, T):
    h64, e64, e_ref32 = SO.reference(weights, inputs, N, T)
    embeds, hidden = run(weights, SO.frames(inputs, N, T), want_hidden=True)
    assert embeds.shape == e64.shape and hidden.shape == h64.shape and embeds.dtype == hidden.dtype == torch.float32
    assert bool(torch.isfinite(embeds).all()) and bool(torch.isfinite(hidden).all())
    e_h, e_e = float((hidden.double() - h64).abs().max()), float((embeds.double() - e64).abs().max())
    e_kernel = max(e_h, e_e)
    print("\n%-7s %-5s N=%-2d T=%-4d e_kernel %.2e (hidden %.2e embeds %.2e)  e_ref32 %.2e  ratio %.2f"
          % (weights, inputs, N, T, e_kernel, e_h, e_e, e_ref32, e_kernel / max(e_ref32, 1e-30)))
    assert e_h <= 1e-3 and e_e <= 1e-3
    assert e_kernel <= 4 * e_ref32 + 2e-6
    assert float((embeds.double().norm(dim=1) - 1).abs().max()) <= 1e-5


@pytest.mark.parametrize("inputs", SO.INPUTS)
def test_rows_do_not_depend_on_the_batch(run, inputs):
    x = SO.frames(inputs, 17, 160)
    embeds, hidden = run("default", x, want_hidden=True)
    for n in range(17):
        e1, h1 = run("default", x[n:n + 1], want_hidden=True)
        assert torch.equal(e1, embeds[n:n + 1]) and torch.equal(h1, hidden[n:n + 1]), n


def test_partials_are_addressed_not_copied(run):
    """P = 4, S = 80, T = 160 on frames [2, 400, 40] against the eight slices stacked and run as plain sequences: bit for bit; and the
    utterance embedding against the float64 mean and renormalisation."""
    x = SO.frames("noise", 2, 400)
    embeds, hidden, utt = run("default", x, P=4, S=80, T=160, want_hidden=True, want_utt=True)
    stacked = torch.stack([x[u, 80 * p:80 * p + 160] for u in range(2) for p in range(4)])
    e1, h1 = run("default", stacked, want_hidden=True)
    assert tuple(embeds.shape) == (8, 256) and tuple(utt.shape) == (2, 256)
    assert torch.equal(embeds, e1) and torch.equal(hidden, h1)
    _, e64 = SO.run_torch(SO.state("default"), stacked, torch.float64)
    assert float((embeds.double() - e64).abs().max()) <= 1e-3
    assert float((utt.double() - SO.utt_reference(e64, 2, 4)).abs().max()) <= 1e-3
    # the last row the geometry may touch is row 399; one frame more is refused on the host
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        run("default", x, P=4, S=80, T=161)


def test_an_all_zero_embedding_is_nan_as_in_the_reference(S, dev):
    sd = SO.state("default")
    sd["linear.bias"] = torch.full_like(sd["linear.bias"], -10.0)
    x = SO.frames("noise", 3, 7)
    plan = S.SpkPlan()
    embeds, hidden = plan.forward(plan.pack(sd, dev), x.to(dev), want_hidden=True)
    h32, e32 = SO.run_torch(sd, x, torch.float32)
    assert bool(torch.isnan(embeds).all()) and bool(torch.isnan(e32).all())
    assert bool(torch.isfinite(hidden).all()) and float((hidden.cpu() - h32).abs().max()) <= 1e-3


# ---- the drop-in package
@pytest.fixture(scope="module")
def I(dev, tmp_path_factory):
    mod = SO.encoder_pkg()
    sd = SO.state("default")
    sd.update(similarity_weight=torch.tensor([10.]), similarity_bias=torch.tensor([-5.]))
    path = tmp_path_factory.mktemp("spk") / "encoder.pt"
    torch.save({"model_state": sd, "step": 3}, path)
    mod.load_model(path, device=dev)
    assert mod.is_loaded()
    return mod


@pytest.mark.parametrize("seconds", [2.3, 10.0])
def test_embed_utterance(I, seconds):
    wav = I.preprocess_wav(SO.harmonic_wav(int(16000 * seconds), 150.0, seed=5), trim_silence=False)
    want, want_partials = SO.utterance_recipe(SO.state("default"), wav)
    embed = I.embed_utterance(wav)
    assert isinstance(embed, np.ndarray) and embed.shape == (256,) and embed.dtype == np.float32
    assert abs(float(np.linalg.norm(embed.astype(np.float64))) - 1) <= 1e-5
    assert float(np.abs(embed - want).max()) <= 1e-3
    embed2, partials, wave_slices = I.embed_utterance(wav, return_partials=True)
    assert np.array_equal(embed2, embed) and partials.shape == want_partials.shape and partials.dtype == np.float32
    assert float(np.abs(partials - want_partials).max()) <= 1e-3
    assert wave_slices == I.compute_partial_slices(len(wav))[0]
    whole, none1, none2 = I.embed_utterance(wav, using_partials=False, return_partials=True)
    assert none1 is None and none2 is None and whole.shape == (256,)
    assert float(np.abs(whole - SO.utterance_recipe(SO.state("default"), wav, using_partials=False)[0]).max()) <= 1e-3


@pytest.mark.parametrize("L", [40000, 46000])
def test_embed_utterance_batch(I, dev, L):
    """[3, 40000] drops its last partial; [3, 46000] keeps it and is padded -- with ones, as the reference pads a batch."""
    wavs = torch.from_numpy(np.stack([SO.harmonic_wav(L, 120.0 + 30 * b, seed=20 + b) for b in range(3)]))
    embeds, partials, wave_slices = I.embed_utterance_batch(wavs.to(dev), return_partials=True)
    assert embeds.is_cuda and tuple(embeds.shape) == (3, 256) and tuple(partials.shape) == (3, len(wave_slices), 256)
    assert (wave_slices[-1].stop > L) == (L == 46000)
    for b in range(3):
        want, want_partials = SO.utterance_recipe(SO.state("default"), wavs[b].numpy(), pad_value=1.0)
        assert float(np.abs(embeds[b].cpu().numpy() - want).max()) <= 1e-3
        assert float(np.abs(partials[b].cpu().numpy() - want_partials).max()) <= 1e-3
    assert torch.equal(I.embed_utterance_batch(wavs.to(dev)), embeds)


def test_changed_weights_are_packed_again(I, dev):
    """Runs last among the drop-in tests: it edits the loaded model."""
    x = SO.frames("noise", 3, 7)
    before = I.embed_frames_batch(x.numpy())
    blob = I._model._hip_packed[str(dev)][2]
    assert np.array_equal(I.embed_frames_batch(x.numpy()), before) and I._model._hip_packed[str(dev)][2] is blob      # cached
    I._model.linear.weight.data.mul_(2)                   # a write through .data bumps no version counter
    after = I.embed_frames_batch(x.numpy())
    assert I._model._hip_packed[str(dev)][2] is not blob
    sd = SO.state("default")
    sd["linear.weight"] = sd["linear.weight"] * 2
    assert not np.array_equal(after, before)
    assert float(np.abs(after - SO.run_torch(sd, x, torch.float64)[1].numpy()).max()) <= 1e-3
    I._model.linear.weight.data.mul_(0.5)


def test_one_call_allocates_its_outputs_only(S, dev):
    """Beyond the packed blob and the cached workspace a call allocates its outputs and nothing else, not even transiently."""
    plan = S.SpkPlan()
    blob = plan.pack(SO.state("default"), dev)
    x = SO.frames("noise", 2, 400).to(dev)
    kw = dict(P=4, S=80, T=160, want_hidden=True, want_utt=True)
    plan.forward(blob, x, **kw)                           # (first call: code object load, workspace)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    out = plan.forward(blob, x, **kw)
    torch.cuda.synchronize()
    out_bytes = sum((o.numel() * 4 + 511) // 512 * 512 for o in out)      # the caching allocator hands out multiples of 512 bytes
    assert [tuple(o.shape) for o in out] == [(8, 256), (8, 256), (2, 256)]
    assert torch.cuda.memory_allocated(dev) - before == out_bytes
    assert torch.cuda.max_memory_allocated(dev) - before == out_bytes
    del out
    assert torch.cuda.memory_allocated(dev) == before
