"""Regenerate tests/golden/ge2e.npz from the reference's own SpeakerEncoder.loss (DiffVC/speaker_encoder/encoder/model.py:65-137) on the
CPU, run where the reference tree is mounted:

    python tests/golden/make_golden_ge2e.py [path to DiffVC/speaker_encoder]

The reference fills its similarity matrix with np.int, which current numpy no longer has: this script sets np.int = int for the run.
Modules the reference imports at the top and that are absent are stubbed as in make_golden_spk.py; sklearn and scipy must be present
(the EER is theirs).  Inputs are tests/ge2e_oracle.embeddings; the file holds data only -- per case `<kind>_<S>_<U>_<name>` for name in
sim, loss, eer, d_embeds, dw, db, checksum (float64, of the regenerated input)."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ge2e_oracle as GO  # noqa: E402

OUT = os.path.join(HERE, "ge2e.npz")
SHAPES = [(2, 2), (3, 4), (8, 5)]
STUBS = ["librosa", "librosa.filters", "webrtcvad", "torchaudio", "torchaudio.transforms", "matplotlib", "matplotlib.pyplot"]


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/DiffVC/speaker_encoder"
    sys.path.insert(0, root)
    for name in STUBS:
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = _Stub(name)
    if not hasattr(np, "int"):
        np.int = int
    ref = importlib.import_module("encoder.model")
    cpu = torch.device("cpu")
    out = {}
    for kind in GO.KINDS:
        for S, U in SHAPES:
            model = ref.SpeakerEncoder(cpu, cpu)
            e = GO.embeddings(kind, S, U).clone().requires_grad_(True)
            loss, eer = model.loss(e)
            loss.backward()
            with torch.no_grad():
                sim = model.similarity_matrix(e).reshape(S * U, S)
            key = "%s_%d_%d_" % (kind, S, U)
            out[key + "sim"] = sim.numpy()
            out[key + "loss"] = np.float32(loss.item())
            out[key + "eer"] = np.float64(eer)
            out[key + "d_embeds"] = e.grad.numpy()
            out[key + "dw"] = model.similarity_weight.grad.numpy()
            out[key + "db"] = model.similarity_bias.grad.numpy()
            out[key + "checksum"] = np.float64(GO.checksum(e.detach()))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d arrays, %d bytes)" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
