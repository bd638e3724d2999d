#!/usr/bin/env python
"""Timing of Fast Griffin-Lim: the HIP kernel path of diffvc/model/utils.py:FastGL against the same module's torch recipe (rocFFT stft,
element-wise phase / momentum ops, istft) on the same GPU, at B = 1 and B = 16, T = 1024 frames, n_iters = 32 (n_fft 1024, 80 mels,
hop 256: 11.9 s of audio per row).

  python tools/fgl_prof.py [--calls 20] [--out fgl.json]
      device events around every call, every shape warmed up, the two legs alternated call by call in one process; reports the median,
      the quartiles and the extremes per leg, their ratio, the kernel path's time per iteration, and the spectral convergence of both
      results (the waveforms themselves differ: two float32 trajectories diverge).
A missing GPU is an error."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CFG = (80, 22050, 1024, 256)            # n_mels, sampling_rate, n_fft, hop_size
SIZES = ((1, 1024), (16, 1024))
N_ITERS = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fgl_prof.py needs a GPU")
    U = importlib.import_module("speech-backbones_amd.diffvc.model.utils")
    MD = importlib.import_module("speech-backbones_amd.hifi_gan.meldataset")
    dev = torch.device("cuda:0")
    g = U.FastGL(*CFG).to(dev)
    n_mels, sr, n_fft, hop = CFG
    result = {"config": list(CFG), "n_iters": N_ITERS, "calls": a.calls, "sizes": []}
    for B, T in SIZES:
        t = torch.arange(hop * T, dtype=torch.float64) / sr           # a vibrato harmonic tone plus noise: a mel with structure
        rows = [sum(torch.sin(h * 2 * torch.pi * (110.0 + 7.0 * b) * t) / h for h in range(1, 30)) for b in range(B)]
        y = torch.stack(rows)
        y = (0.9 * y / y.abs().max() + 1e-3 * torch.randn(B, hop * T, generator=torch.Generator().manual_seed(B), dtype=torch.float64))
        mel = MD.mel_spectrogram(y.float().to(dev), n_fft, n_mels, sr, hop, n_fft, 0, 8000)
        assert mel.shape[-1] == T
        run = {"kernel": lambda: g(mel, n_iters=N_ITERS), "torch": lambda: torch_leg(g, mel)}
        outs = {}
        for name, fn in run.items():                                  # warm-up: code objects, rocFFT plans, packed tables
            for _ in range(2):
                outs[name] = fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in run}
        for _ in range(max(5, a.calls)):
            for name, fn in run.items():                              # alternated: both legs see the same clocks and neighbours
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        c = g.pi(mel).double()
        entry = {"B": B, "T": T, "samples_per_row": hop * (T - 1)}
        for name, v in ms.items():
            q = statistics.quantiles(v, n=4)
            entry[name + "_ms"] = {"median": statistics.median(v), "q1": q[0], "q3": q[2], "min": min(v), "max": max(v), "n": len(v)}
            x = outs[name][:, 0].double()
            mag = torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=g.window.double(), center=True, return_complex=True).abs()
            entry[name + "_spectral_convergence"] = float(torch.linalg.norm(mag - c) / torch.linalg.norm(c))
        entry["torch_over_kernel"] = entry["torch_ms"]["median"] / entry["kernel_ms"]["median"]
        entry["kernel_us_per_iteration"] = 1e3 * entry["kernel_ms"]["median"] / N_ITERS
        result["sizes"].append(entry)
        print(json.dumps(entry))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


def torch_leg(g, mel):
    """The module's own torch recipe on the device in float32 (forward() itself sends such a tensor to the kernels)."""
    import torch
    with torch.no_grad():
        return g._torch_recipe(mel, N_ITERS)


if __name__ == "__main__":
    main()
