"""GPU parity tests (-m gpu) of the encoder kernels (csrc/enc.hip) through the C ABI: TextEncoder and MelEncoder against the
reference's golden outputs and the CPU oracle.  Tolerance: max|err| <= 1e-4 * max|ref| (split-bf16 convolutions, fp32
attention / LayerNorm)."""
import importlib

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import encoder_oracle as E
from case_util import relerr_floor as relerr
from gpu_guards import S, dev  # noqa: F401

pytestmark = pytest.mark.gpu
REL = 1e-4


def _t(a):
    return torch.from_numpy(np.asarray(a))


def test_text_encoder_matches_reference_golden(S, dev):
    g = golden("encoder.npz")
    sd = E.make_state("text", seed=0)
    enc = S.Encoder("text")
    blob = enc.pack(sd, dev)
    ids, lens = _t(g["text_ids"]), _t(g["text_lens"])
    mask = E.sequence_mask(lens, ids.shape[1]).unsqueeze(1).float()
    mu, logw = enc.forward(blob, ids.to(dev), mask.to(dev))
    print("text encoder: mu rel %.2e, logw rel %.2e" % (relerr(mu.cpu(), _t(g["text_mu"])), relerr(logw.cpu(), _t(g["text_logw"]))))
    assert relerr(mu.cpu(), _t(g["text_mu"])) <= REL and relerr(logw.cpu(), _t(g["text_logw"])) <= REL
    assert float((mu.cpu() * (1 - mask)).abs().max()) == 0.0 and float((logw.cpu() * (1 - mask)).abs().max()) == 0.0


def test_mel_encoder_matches_reference_golden(S, dev):
    g = golden("encoder.npz")
    sd = E.make_state("mel", seed=2)
    enc = S.Encoder("mel", 0, 80, 192, 768, 0, 2, 6, 3, 4)
    out = enc.forward(enc.pack(sd, dev), _t(g["mel_in"]).to(dev), _t(g["mel_mask"]).to(dev)).cpu()
    assert relerr(out, _t(g["mel_out"])) <= REL


@pytest.mark.parametrize("B,L", [(1, 1), (2, 7), (3, 130), (2, 301)])
def test_text_encoder_matches_oracle_shapes(S, dev, B, L):
    """Sequence lengths around the relative window (L <= 5), across attention / conv tiles, ragged batches, a 1-token item."""
    sd = E.make_state("text", seed=7)
    enc = S.Encoder("text")
    g = torch.Generator().manual_seed(L)
    ids = torch.randint(0, 149, (B, L), generator=g)
    lens = torch.tensor([L] + [max(1, L // (k + 2)) for k in range(B - 1)])
    mu_o, logw_o, mask = E.text_encoder_forward(sd, ids, lens)
    mu, logw = enc.forward(enc.pack(sd, dev), ids.to(dev), mask.to(dev))
    assert relerr(mu.cpu(), mu_o) <= REL
    # log-durations are O(1) sums of 256 signed terms; a 1-token batch has a single (possibly tiny) value, so the bound
    # is taken on the O(1) scale of the quantity rather than on that one value
    assert float((logw.cpu() - logw_o).abs().max()) <= REL * max(1.0, float(logw_o.abs().max()))


def test_text_encoder_module_uses_the_kernels_in_inference(S, dev):
    """TextEncoder.forward in eval mode under no_grad on HIP tensors runs gtts_enc_forward; the same module with autograd
    enabled composes torch ops -- both against the oracle."""
    TE = importlib.import_module("speech-backbones_amd.model.text_encoder")
    sd = E.make_state("text", seed=8)
    enc = TE.TextEncoder(149, 80, 192, 768, 256, 2, 6, 3, 0.1, 4)
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev).eval()
    ids = torch.randint(0, 149, (2, 33))
    lens = torch.tensor([33, 20])
    mu_o, logw_o, mask_o = E.text_encoder_forward(sd, ids, lens)
    with torch.no_grad():
        mu, logw, mask = enc(ids.to(dev), lens.to(dev))
    assert enc._hip_blob is not None
    assert torch.equal(mask.cpu(), mask_o) and relerr(mu.cpu(), mu_o) <= REL and relerr(logw.cpu(), logw_o) <= REL
    mu_t, logw_t, _ = enc(ids.to(dev), lens.to(dev))          # grad enabled: torch composition
    assert relerr(mu_t.detach().cpu(), mu_o) <= 1e-4
    ME = importlib.import_module("speech-backbones_amd.diffvc.model.encoder")
    sdm = E.make_state("mel", seed=9)
    menc = ME.MelEncoder(80, 192, 768, 2, 6, 3, 0.1, window_size=4)
    menc.load_state_dict(sdm, strict=True)
    menc = menc.to(dev).eval()
    mel = torch.randn(2, 80, 52)
    mm = E.sequence_mask(torch.tensor([52, 31]), 52).unsqueeze(1).float()
    with torch.no_grad():
        out = menc(mel.to(dev), mm.to(dev)).cpu()
    assert relerr(out, E.mel_encoder_forward(sdm, mel, mm)) <= REL


@pytest.mark.parametrize("B,T", [(2, 45), (1, 7), (2, 130)])
def test_postnet_matches_reference_and_oracle(S, dev, B, T):
    """DiffVC PostNet (7x7 MFMA convolutions with fused GroupNorm statistics, Mish-on-load, EPI_TAIL residual) against the
    reference's golden output (B=2, T=45) and the CPU oracle at other shapes."""
    from oracle import postnet_oracle as P
    sd = P.make_state(128, seed=0)
    plan = S.PostNetPlan(128)
    blob = plan.pack(sd, dev)
    if (B, T) == (2, 45):
        g = golden("postnet.npz")
        x, mask, ref = _t(g["x"]), _t(g["mask"]), _t(g["y"])
    else:
        gen = torch.Generator().manual_seed(T)
        x = torch.randn(B, 80, T, generator=gen)
        mask = E.sequence_mask(torch.tensor([T] + [max(1, T // 2)] * (B - 1)), T).unsqueeze(1).float()
        ref = P.postnet_forward(sd, x, mask)
    out = plan.forward(blob, x.to(dev), mask.to(dev)).cpu()
    print("postnet B=%d T=%d rel err %.2e" % (B, T, relerr(out, ref)))
    assert relerr(out, ref) <= REL
    PN = importlib.import_module("speech-backbones_amd.diffvc.model.postnet")
    net = PN.PostNet(128)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    with torch.no_grad():
        assert relerr(net(x.to(dev), mask.to(dev)).cpu(), ref) <= REL


@pytest.mark.parametrize("length_scale", [0.91, 1.0])
def test_duration_ceil_flips_against_the_cpu_encoder(S, dev, length_scale):
    """Alignment fragility (Grad-TTS/model/tts.py:77-86): w_ceil = ceil(exp(logw) * x_mask) * length_scale is a
    discontinuous function of the encoder's log-durations, so a 1e-5 difference between the HIP encoder and the CPU one can move a
    token's duration by a whole frame.  Identical token ids and weights through both encoders, B = 16 utterances of 50-300 tokens:
    the test REPORTS the number of tokens whose ceil differs (the flip rate quoted in DESIGN.md) and asserts what must hold --
    every flip sits within the encoders' 1e-4 tolerance of an integer boundary, a flip moves a duration by exactly one frame, and
    y_lengths agree exactly for every utterance without a flip."""
    sd = E.make_state("text", seed=11)
    enc = S.Encoder("text")
    blob = enc.pack(sd, dev)
    g = torch.Generator().manual_seed(2024)
    B = 16
    lens = torch.randint(50, 301, (B,), generator=g)
    L = int(lens.max())
    ids = torch.randint(0, 149, (B, L), generator=g)
    _, logw_o, mask = E.text_encoder_forward(sd, ids, lens)
    _, logw = enc.forward(blob, ids.to(dev), mask.to(dev))
    logw = logw.cpu()
    w_o, w_h = torch.exp(logw_o) * mask, torch.exp(logw) * mask
    c_o, c_h = torch.ceil(w_o) * length_scale, torch.ceil(w_h) * length_scale
    flips = (c_o != c_h) & (mask > 0)
    n_tok, n_flip = int(mask.sum()), int(flips.sum())
    y_o = torch.clamp_min(torch.sum(c_o, [1, 2]), 1).long()
    y_h = torch.clamp_min(torch.sum(c_h, [1, 2]), 1).long()
    print("length_scale %.2f: %d of %d tokens have a different ceil(exp(logw)) on the HIP encoder (max |logw diff| %.2e); "
          "y_lengths differ for %d of %d utterances" % (length_scale, n_flip, n_tok, float((logw - logw_o).abs().max()),
                                                       int((y_o != y_h).sum()), B))
    if n_flip:
        # a flip needs the duration within the encoders' relative tolerance of an integer, and moves it by one frame
        near = (w_o[flips] - torch.round(w_o[flips])).abs() / w_o[flips].clamp_min(1.0)
        assert float(near.max()) <= 2e-4
        assert float((torch.ceil(w_o)[flips] - torch.ceil(w_h)[flips]).abs().max()) == 1.0
    per_utt = flips.flatten(1).sum(1)
    assert torch.equal(y_o[per_utt == 0], y_h[per_utt == 0])
    assert n_flip <= 2            # expected 0: P(|w - round(w)| < 1e-5 w) ~ 1e-5 per token, ~2 800 tokens
