"""Regenerate tests/golden/spk_partial_slices.json from the reference's own compute_partial_slices
(DiffVC/speaker_encoder/encoder/inference.py:57-108), run where the reference tree is mounted:

    python tests/golden/make_golden_spk.py [path to DiffVC/speaker_encoder]

The reference module imports librosa, webrtcvad, torchaudio, scipy, sklearn and matplotlib at the top; none of them is touched by the
function recorded here, so whichever is missing is replaced by an empty stub module for the import.  The file holds data only:
for every case the arguments and the [start, stop] pairs of the wav and mel slices."""
import importlib
import json
import os
import sys
import types

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "spk_partial_slices.json")
N_SAMPLES = [1, 159, 25600, 25601, 38399, 38400, 160000, 16000 * 37 + 11]
VARIANTS = [{}, {"overlap": 0.25}, {"overlap": 0.0, "min_pad_coverage": 0.5}, {"min_pad_coverage": 1.0},
            {"partial_utterance_n_frames": 80, "overlap": 0.9, "min_pad_coverage": 0.1}]
STUBS = ["librosa", "librosa.filters", "webrtcvad", "torchaudio", "torchaudio.transforms", "scipy", "scipy.ndimage",
         "scipy.ndimage.morphology", "scipy.interpolate", "scipy.optimize", "sklearn", "sklearn.metrics", "matplotlib",
         "matplotlib.pyplot"]


class _Stub(types.ModuleType):
    def __getattr__(self, name):            # `from x import y` of a stubbed module yields a placeholder nobody calls
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
    ref = importlib.import_module("encoder.inference")
    cases = []
    for kw in VARIANTS:
        for n in N_SAMPLES:
            wav, mel = ref.compute_partial_slices(n, **kw)
            cases.append({"n_samples": n, "kwargs": kw, "wav": [[int(s.start), int(s.stop)] for s in wav],
                          "mel": [[int(s.start), int(s.stop)] for s in mel]})
    with open(OUT, "w") as f:
        json.dump({"source": "DiffVC/speaker_encoder/encoder/inference.py compute_partial_slices", "cases": cases}, f, separators=(",", ":"))
    print("wrote %s (%d cases)" % (OUT, len(cases)))


if __name__ == "__main__":
    main()
