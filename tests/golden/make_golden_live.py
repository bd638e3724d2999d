"""Regenerate tests/golden/live_*.npz: what the reference's OWN modules return in the comparisons that the CPU tests used to make
live against the reference tree (test_oracle_vs_reference.py, test_diffvc_shell_cpu.py, test_model_cpu.py, test_encoder_cpu.py,
test_hifigan_cpu.py, test_oracle_golden.py) and in the compiled-MAS comparison of test_gpu_parity.py.

Run where the reference tree is mounted:  python tests/golden/make_golden_live.py

Weights are not stored where the product's modules reproduce the reference's default initialisation under the same seed:
the file keeps the reference's layout and a per-tensor |.|-sum instead, and the tests check that their own modules match it.
Inputs drawn from the global RNG are stored.  Parameter gradients, and the HiFi-GAN weights with weight norm folded, are kept
as per-tensor summaries (gradients: norm and max |.|; weights: |.|-sum) plus 64 entries at fixed positions per tensor (all
entries of smaller tensors), in float32.  The arrays are split over files by key prefix (live_golden.GROUPS)."""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import encoder_oracle as E  # noqa: E402
from oracle import gradtts_oracle as O  # noqa: E402
from oracle import hifigan_oracle as H  # noqa: E402
from oracle import mas as MAS  # noqa: E402
from oracle import ref_loader  # noqa: E402
import live_golden as L  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def put_state(out, tag, sd):
    out[tag + "_names"], out[tag + "_shapes"] = L.encode_layout(sd)
    out[tag + "_abssum"] = np.array([float(v.double().abs().sum()) for v in sd.values()])


def main():
    torch.set_num_threads(L.GOLDEN_THREADS)
    out = {}
    gt = ref_loader.load_gradtts()

    # test_oracle_vs_reference.py
    for n_spks in (1, 5):
        dec = gt.diffusion.Diffusion(80, 64, n_spks, 64, 0.05, 20.0, 1000)
        est = {k[len("estimator."):]: v for k, v in dec.state_dict().items()}
        out["est_layout_s%d_names" % n_spks], out["est_layout_s%d_shapes" % n_spks] = L.encode_layout(est)
    torch.manual_seed(0)
    sd = O.make_estimator_state(seed=7)
    dec = gt.diffusion.Diffusion(80, 64, 1, 64, 0.05, 20.0, 1000)
    dec.estimator.load_state_dict(sd, strict=True)
    inp = O.make_inputs(2, 48, seed=3)
    with torch.no_grad():
        out["est_taps_out"] = dec.estimator(inp["z"], inp["mask"], inp["mu"], torch.tensor([0.15, 0.95])).numpy()
    sd = O.make_estimator_state(seed=1)
    dec = gt.diffusion.Diffusion(80, 64, 1, 64, 0.05, 20.0, 1000)
    dec.estimator.load_state_dict(sd, strict=True)
    inp = O.make_inputs(1, 32, seed=4)
    with torch.no_grad():
        out["rd3_out"] = dec(inp["z"], inp["mask"], inp["mu"], 3).numpy()

    # test_model_cpu.py::test_whole_model_against_reference_live
    ARGS = (149, 1, 64, 192, 768, 256, 2, 6, 3, 0.1, 4, 80, 64, 0.05, 20.0, 1000)
    torch.manual_seed(0)
    r = gt.GradTTS(*ARGS).eval()
    put_state(out, "gradtts", r.state_dict())
    x = torch.randint(0, 149, (2, 37))
    xl = torch.tensor([37, 21])
    out["gradtts_x"] = x.numpy()
    with torch.no_grad():
        for i, a in enumerate(r.encoder(x, xl)):
            out["gradtts_enc%d" % i] = a.numpy()
    y = torch.randn(2, 80, 60)
    out["gradtts_y"] = y.numpy()
    for out_size in (None, 48, 52):
        random.seed(5)
        torch.manual_seed(1)
        for i, a in enumerate(r.compute_loss(x, xl, y, torch.tensor([60, 44]), out_size=out_size)):
            out["gradtts_loss_%s_%d" % (out_size, i)] = a.detach().numpy()

    # test_model_cpu.py::test_parameter_gradients_match_reference_loss_t
    for n_spks in (1, 3):
        tag = "grad_s%d" % n_spks
        sd = O.make_estimator_state(n_spks=n_spks, seed=11)
        theirs = gt.diffusion.Diffusion(80, 64, n_spks, 64, 0.05, 20.0, 1000)
        theirs.estimator.load_state_dict(sd, strict=True)
        inp = O.make_inputs(2, 36, seed=2, spk_dim=64 if n_spks > 1 else None)
        torch.manual_seed(4)
        la, xta = theirs.loss_t(inp["z"], inp["mask"], inp["mu"], torch.tensor([0.35, 0.8]), inp.get("spk"))
        la.backward()
        out[tag + "_loss"], out[tag + "_xt"] = la.detach().numpy(), xta.detach().numpy()
        grads = {n: p.grad for n, p in theirs.estimator.named_parameters()}
        out[tag + "_names"] = np.array(list(grads))
        out[tag + "_has_grad"] = np.array([g is not None for g in grads.values()])
        sel = [g.detach().double().flatten().numpy() for g in grads.values() if g is not None]
        out[tag + "_norm"] = np.array([np.sqrt((g * g).sum()) for g in sel])
        out[tag + "_max"] = np.array([np.abs(g).max() for g in sel])
        out[tag + "_vals"] = np.concatenate([g[L.sample_index(g.size)] for g in sel]).astype(np.float32)

    # test_encoder_cpu.py::test_oracle_against_reference_live
    sd = E.make_state("text", seed=5)
    enc = gt.text_encoder.TextEncoder(149, 80, 192, 768, 256, 2, 6, 3, 0.1, 4).eval()
    enc.load_state_dict(sd, strict=True)
    ids = torch.randint(0, 149, (2, 50))
    out["textenc_ids"] = ids.numpy()
    with torch.no_grad():
        for k, a in zip(("mu", "logw", "mask"), enc(ids, torch.tensor([50, 1]))):
            out["textenc_" + k] = a.numpy()

    # test_diffvc_shell_cpu.py
    vc = ref_loader.load_diffvc()
    torch.manual_seed(0)
    r = vc.vc.DiffVC(*L.VC_ARGS.values()).eval()
    put_state(out, "vc", r.state_dict())
    out["vc_enc_names"], out["vc_enc_shapes"] = L.encode_layout(r.encoder.state_dict())
    out["vc_nparams"] = np.int64(r.nparams)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 80, 44, generator=g)
    mask = (torch.arange(44)[None, :] < torch.tensor([44, 31])[:, None]).unsqueeze(1).float()
    y = torch.randn(2, 80, 44, generator=g)
    out["vc_avg_voice"] = r.encoder(x, mask).detach().numpy()
    out["vc_avg_voice_loss"] = r.encoder.compute_loss(x, y, mask).detach().numpy()
    got = {}

    def recorder(z, mask, mean, ref, ref_mask, mean_ref, c_, n_timesteps, mode):
        got.update(z=z, mask=mask, mean=mean, ref=ref, ref_mask=ref_mask, mean_ref=mean_ref, c=c_)
        out["vc_fwd_n"], out["vc_fwd_mode"] = np.int64(n_timesteps), np.array(mode)
        return z * 2.0

    r.decoder.forward = recorder
    x, x_len, x_ref, r_len, c = L.vc_forward_inputs()
    torch.manual_seed(11)
    ra = r(x, x_len, x_ref, r_len, c, 6, "ml")
    for k, v in got.items():
        out["vc_fwd_" + k] = v.detach().numpy()
    out["vc_fwd_out0"], out["vc_fwd_out1"] = ra[0].detach().numpy(), ra[1].detach().numpy()
    del r.decoder.forward
    x, x_len, x_ref, c = L.vc_loss_inputs()
    torch.manual_seed(2)
    out["vc_loss"] = r.compute_loss(x, x_len, x_ref, c).detach().numpy()

    # test_hifigan_cpu.py::test_oracle_and_module_against_reference_live
    hf = ref_loader.load_hifigan()
    torch.manual_seed(0)
    r = hf.Generator(hf.AttrDict(L.hifigan_attr(H.SMALL)))
    put_state(out, "hifigan", r.state_dict())
    with torch.no_grad():
        out["hifigan_wav"] = r(H.make_mel(2, 9, seed=1)).numpy()
    r.remove_weight_norm()
    eff = r.state_dict()
    out["hifigan_eff_names"], out["hifigan_eff_shapes"] = L.encode_layout(eff)
    out["hifigan_eff_abssum"] = np.array([float(v.double().abs().sum()) for v in eff.values()])
    out["hifigan_eff_vals"] = np.concatenate([v.detach().flatten().numpy()[L.sample_index(v.numel())] for v in eff.values()])

    # test_oracle_golden.py / test_gpu_parity.py: the compiled reference MAS
    for i, (value, mask) in enumerate(L.mas_random_cases()):
        out["mas_rand%d" % i] = MAS.maximum_path_ref(value, mask).to(torch.uint8).numpy()
    value, mask = L.mas_gpu_case()
    out["mas_gpu"] = MAS.maximum_path_ref(value, mask).to(torch.uint8).numpy()

    files = {}
    for k, v in out.items():
        files.setdefault(L.group_of(k), {})[k] = v
    for name, arrays in files.items():
        path = os.path.join(OUT, "live_%s.npz" % name)
        np.savez_compressed(path, **arrays)
        print("written", path, len(arrays), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
