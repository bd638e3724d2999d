"""Regenerate tests/golden/enc_loss_grads.npz from the reference's OWN DiffVC "average voice" encoder run on CPU: FwdDiffusion.compute_loss
(DiffVC/model/vc.py:43-48, what DiffVC/train_enc.py:83-91 optimises; the reference's own FwdDiffusion) and the gradient of its loss w.r.t. every parameter, at enc_dim 128.

Run in the build container (where /root/reference is mounted):  python tests/golden/make_golden_grads_enc.py
The module is in eval() mode (dropout off) with autograd on.  Weights are re-derived from oracle.encoder_oracle.make_state("mel", seed)
and oracle.postnet_oracle.make_state(dim, seed) (checksum kept).  Per parameter the file keeps the gradient's L2 norm, its max |.| and
16 entries at fixed positions; the gradient w.r.t. the PostNet's input is kept the same way (`z_*`)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import encoder_oracle as E  # noqa: E402
from oracle import postnet_oracle as P  # noqa: E402
from oracle import ref_loader  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
NS = 16
DIM, B, T = 128, 2, 48
SEED_ENC, SEED_PN, SEED_IN = 11, 12, 13


def sample_index(n):
    return np.unique(np.linspace(0, n - 1, NS).round().astype(np.int64))


def make_state():
    sd = {"encoder." + k: v for k, v in E.make_state("mel", seed=SEED_ENC).items()}
    sd.update({"postnet." + k: v for k, v in P.make_state(DIM, seed=SEED_PN).items()})
    return sd


def make_inputs():
    g = torch.Generator().manual_seed(SEED_IN)
    mask = torch.ones(B, 1, T)
    mask[1, :, 37:] = 0                                   # ragged: the second utterance is 37 frames
    x = torch.randn(B, 80, T, generator=g) * mask
    y = torch.randn(B, 80, T, generator=g) * mask
    return {"x": x, "y": y, "mask": mask}


def summarise(g):
    g = g.detach().double().flatten().numpy()
    idx = sample_index(g.size)
    v = np.zeros(NS)
    v[:idx.size] = g[idx]
    return np.sqrt((g * g).sum()), np.abs(g).max(), v


def main():
    ref = ref_loader.load_diffvc()
    fwd = ref.vc.FwdDiffusion(80, 192, 768, 2, 6, 3, 0.1, 4, DIM)
    sd = make_state()
    fwd.load_state_dict(sd, strict=True)
    fwd.eval()
    inp = make_inputs()
    # the reference's own FwdDiffusion.compute_loss (vc.py:43-48); a forward pre-hook on its postnet keeps the PostNet's input z (the
    # MelEncoder's output) so that d loss / d z is recorded as well
    kept = {}

    def keep_input(mod, args):
        args[0].retain_grad()
        kept["z"] = args[0]
    hook = fwd.postnet.register_forward_pre_hook(keep_input)
    loss = fwd.compute_loss(inp["x"], inp["y"], inp["mask"])
    loss.backward()
    hook.remove()
    z = kept["z"]
    enc, pn = fwd.encoder, fwd.postnet
    out = {"checksum": np.float64(sum(float(v.double().abs().sum()) for v in sd.values())), "loss": np.float64(float(loss.detach())),
           "seeds": np.array([SEED_ENC, SEED_PN, SEED_IN]), "dim": np.int64(DIM)}
    for k, v in inp.items():
        out[k] = v.numpy()
    out["z_norm"], out["z_max"], out["z_vals"] = summarise(z.grad)
    names, norms, maxs, vals = [], [], [], []
    for prefix, mod in (("encoder.", enc), ("postnet.", pn)):
        for name, p in mod.named_parameters():
            if p.grad is None:
                continue
            n, m, v = summarise(p.grad)
            names.append(prefix + name)
            norms.append(n)
            maxs.append(m)
            vals.append(v)
    out["names"] = np.array(names)
    out["norm"] = np.array(norms)
    out["max"] = np.array(maxs)
    out["vals"] = np.stack(vals)
    print("loss", float(loss.detach()), "parameters with a gradient", len(names))
    np.savez_compressed(os.path.join(OUT, "enc_loss_grads.npz"), **out)


if __name__ == "__main__":
    main()
