#!/usr/bin/env python
"""Timing of the differentiable log-mel: forward + backward of the HIP kernel path of hifi_gan/meldataset.py (csrc/mel.hip and
csrc/mel_train.hip under autograd) against the same module's torch recipe under autograd (pad, rocFFT stft, magnitude, matmul, log and
their backward ops) on the same GPU, at B = 16, L = 8192 (HiFi-GAN's segment_size: 512 frames) and B = 16, L = 256 * 130.

  python tools/mel_train_prof.py [--reps 7] [--calls 20] [--out profiles/mel_train.json]
      what is timed is the HiFi-GAN step's use: mel = mel_spectrogram(y) with y requiring grad, then mel.backward(dmel) with a fixed
      dmel.  Device events around every call, every shape warmed up, the two legs alternated call by call in one process.  A
      repetition is the median of --calls alternated calls; reported per leg: the median of the repetitions, their extremes and
      quartiles (the spread), the ratio of the medians, and the largest difference between the two legs' gradients over the largest
      gradient (a check that both legs computed the same thing, not a test).
A missing GPU is an error."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CFG = (1024, 80, 22050, 256, 1024, 0, 8000)
SIZES = ((16, 8192), (16, 256 * 130))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mel_train_prof.py needs a GPU")
    MD = importlib.import_module("speech-backbones_amd.hifi_gan.meldataset")
    dev = torch.device("cuda:0")
    cfg = (CFG[0], CFG[1], CFG[2], CFG[3], CFG[4], float(CFG[5]), float(CFG[6]))
    result = {"config": list(CFG), "reps": max(5, a.reps), "calls_per_rep": a.calls, "what": "forward + backward, ms per call", "sizes": []}
    for B, L in SIZES:
        y = (0.3 * torch.randn(B, L, generator=torch.Generator().manual_seed(B))).clamp(-1, 1).to(dev).requires_grad_()
        T = MD._plan(cfg).frames(L)
        dmel = torch.randn(B, CFG[1], T, generator=torch.Generator().manual_seed(L)).to(dev)

        def step(forward):
            y.grad = None
            forward().backward(dmel)
            return y.grad

        run = {"kernel": lambda: step(lambda: MD.mel_spectrogram(y, *CFG)), "torch": lambda: step(lambda: MD._torch_recipe(y, cfg, False))}
        grads = {}
        for name, fn in run.items():                      # warm-up: code objects, rocFFT plans, cached tables, allocator blocks
            for _ in range(5):
                grads[name] = fn().clone()
        torch.cuda.synchronize()
        diff = float((grads["kernel"] - grads["torch"]).abs().max() / grads["torch"].abs().max())
        reps = {"kernel": [], "torch": []}
        for _ in range(max(5, a.reps)):
            ms = {"kernel": [], "torch": []}
            for _ in range(a.calls):
                for name, fn in run.items():              # alternated: both legs see the same clocks and neighbours
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ms[name].append(e0.elapsed_time(e1))
            for name in reps:
                reps[name].append(statistics.median(ms[name]))
        entry = {"B": B, "L": L, "T": T, "frames": B * T, "rel_diff_between_legs_gradients": diff}
        for name, v in reps.items():
            q = statistics.quantiles(v, n=4)
            entry[name + "_ms"] = {"median": statistics.median(v), "q1": q[0], "q3": q[2], "min": min(v), "max": max(v), "reps": len(v)}
        entry["torch_over_kernel"] = entry["torch_ms"]["median"] / entry["kernel_ms"]["median"]
        result["sizes"].append(entry)
        print(json.dumps(entry))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
