"""CPU: the DiffVC model shell (speech-backbones_amd/diffvc/model/vc.py) against the reference's `model.vc`
(DiffVC/model/vc.py:17-148): state_dict layout, the average-voice encoder, and the HOST LOGIC of DiffVC.forward
(masks, padding to a multiple of four, the terminal sample `mean_x + randn`) -- the decoder call itself is replaced by a
recorder on both sides, so everything up to the C-ABI sampler is compared bit for bit.  What the reference returned is stored
in tests/golden/live_*.npz (tests/golden/make_golden_live.py); the shell under torch.manual_seed(0) must reproduce the reference's
default initialisation, which the reference's outputs were computed with."""
import importlib

import pytest
import torch

from live_golden import VC_ARGS, assert_reference_init, layout, live, vc_forward_inputs, vc_loss_inputs


def _t(k):
    return torch.from_numpy(live()[k])


@pytest.fixture(scope="module")
def pair():
    V = importlib.import_module("speech-backbones_amd.diffvc.model")
    torch.manual_seed(0)
    p = V.DiffVC(*VC_ARGS.values()).eval()
    return live(), p


def test_state_dict_layout_and_drop_in_load(pair):
    r, p = pair
    assert_reference_init(p.state_dict(), r, "vc")
    p.load_state_dict(p.state_dict(), strict=True)
    assert p.nparams == int(r["vc_nparams"])
    fa = importlib.import_module("speech-backbones_amd.diffvc.model").FwdDiffusion(80, 48, 96, 2, 2, 3, 0.0, 4, 32)
    assert [(k, tuple(v.shape)) for k, v in fa.state_dict().items()] == layout(r, "vc_enc")
    fa.load_state_dict(p.encoder.state_dict(), strict=True)


def test_average_voice_encoder_matches_reference(pair):
    r, p = pair
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 80, 44, generator=g)
    lens = torch.tensor([44, 31])
    mask = (torch.arange(44)[None, :] < lens[:, None]).unsqueeze(1).float()
    a, b = _t("vc_avg_voice"), p.encoder(x, mask)
    assert torch.allclose(a, b, atol=1e-5, rtol=1e-5)
    y = torch.randn(2, 80, 44, generator=g)
    assert torch.allclose(_t("vc_avg_voice_loss"), p.encoder.compute_loss(x, y, mask), atol=1e-6)


def test_forward_host_logic_bit_identical(pair):
    """Everything DiffVC.forward hands to the decoder, and what it returns, with the decoder replaced by a recorder."""
    r, p = pair
    x, x_len, x_ref, r_len, c = vc_forward_inputs()       # longest 50 -> padded to 52
    got = {"ref": {k: _t("vc_fwd_" + k) for k in ("z", "mask", "mean", "ref", "ref_mask", "mean_ref", "c")}}
    got["ref"].update(n=int(r["vc_fwd_n"]), mode=str(r["vc_fwd_mode"]))

    def recorder(tag):
        def fwd(z, mask, mean, ref, ref_mask, mean_ref, c_, n_timesteps, mode):
            got[tag] = dict(z=z.clone(), mask=mask.clone(), mean=mean.clone(), ref=ref.clone(), ref_mask=ref_mask.clone(),
                            mean_ref=mean_ref.clone(), c=c_.clone(), n=n_timesteps, mode=mode)
            return z * 2.0
        return fwd

    p.decoder.forward = recorder("own")
    ra = (_t("vc_fwd_out0"), _t("vc_fwd_out1"))
    torch.manual_seed(11)
    pa = p(x, x_len, x_ref, r_len, c, 6, "ml")
    assert got["ref"]["n"] == got["own"]["n"] == 6 and got["ref"]["mode"] == got["own"]["mode"] == "ml"
    assert got["own"]["z"].shape == (3, 80, 52)
    for k in ("mask", "ref", "ref_mask", "c"):
        assert torch.equal(got["ref"][k], got["own"][k]), k
    for k in ("z", "mean", "mean_ref"):                 # through the (CPU) encoders: same composition, same values
        assert torch.allclose(got["ref"][k], got["own"][k], atol=1e-5, rtol=1e-5), k
    assert ra[1].shape == pa[1].shape == (3, 80, 50)
    assert torch.allclose(ra[0], pa[0], atol=1e-5) and torch.allclose(ra[1], pa[1], atol=1e-5)
    # padded frames carry neither prior mean nor source: only the noise draw
    own = got["own"]
    assert float(own["mean"][1, :, 37:].abs().max()) == 0.0 and float(own["mean"][:, :, 50:].abs().max()) == 0.0


def test_compute_loss_matches_reference(pair):
    r, p = pair
    p.decoder.__dict__.pop("forward", None)
    x, x_len, x_ref, c = vc_loss_inputs()
    a = _t("vc_loss")
    torch.manual_seed(2)
    b = p.compute_loss(x, x_len, x_ref, c)
    assert torch.allclose(a, b, rtol=1e-4, atol=1e-6), (float(a), float(b))
