#!/usr/bin/env python
"""Timing of the speaker encoder's waveform front end: the HIP kernels of csrc/wav.hip against the torch recipes of the drop-in
diffvc/speaker_encoder/encoder/audio.py on the same GPU, at B = 16 x 10 s and B = 1 x 3 s of 22050 Hz audio.

  python tools/wav_prof.py [--calls 50] [--out FILE]          (default: profiles/spk_frontend.json)

Three steps, each a pair of legs: resample (kernel against the strided conv1d -- the parent of this front end had no runnable
resampler), normalise on the resampled waveform (kernel with the resampler's tile sums against the five torch ops), power mel (kernel
against torch.stft + matmul, the path before the kernel).  Device events around every call, every shape warmed up, the two legs
alternated call by call in one process; reports the median, the quartiles and the extremes per leg, their ratio, the launches per call
(device kernels the torch profiler sees in one call) and the kernel leg's bytes/s against the compulsory
traffic (resample 4 B L in + 4 B L' out, normalise 4 B L' in + out, mel 4 B L' in + 4 B T 40 out; reported, no target).
A missing GPU is an error."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SOURCE_SR = 22050
SIZES = ((16, 10 * SOURCE_SR), (1, 3 * SOURCE_SR))


def launches(fn):
    """Device kernels of one call, as the torch profiler records them.  A profiler that records none is an error: the launch count is
    what the comparison rests on."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
            and "memset" not in e.name.lower())
    if n == 0:
        raise SystemExit("wav_prof.py: the profiler recorded no device kernel")
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spk_frontend.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("wav_prof.py needs a GPU")
    A = importlib.import_module("speech-backbones_amd.diffvc.speaker_encoder.encoder.audio")
    dev = torch.device("cuda:0")
    plan, blob = A._plan(SOURCE_SR), A._blob(SOURCE_SR, dev)
    result = {"source_sr": SOURCE_SR, "sampling_rate": A.sampling_rate, "calls": a.calls, "sizes": []}
    for B, L in SIZES:
        x = (0.003 * torch.randn(B, L, generator=torch.Generator().manual_seed(B))).to(dev)       # quieter than -30 dBFS: the gain applies
        y, partials = plan.resample(blob, x)
        Lo, T = y.shape[1], plan.frames(y.shape[1])
        steps = {
            "resample": ({"kernel": lambda: plan.resample(blob, x)[0], "torch": lambda: A.resample_batch(x, SOURCE_SR)},
                         4 * B * L + 4 * B * Lo),
            "normalize": ({"kernel": lambda: plan.normalize(blob, y, A.audio_norm_target_dBFS, True, partials=partials),
                           "torch": lambda: A._normalize_torch(y, A.audio_norm_target_dBFS, True)}, 8 * B * Lo),
            "powmel": ({"kernel": lambda: plan.powmel(blob, y), "torch": lambda: A._mel_torch(y)}, 4 * B * Lo + 4 * B * T * plan.n_mels),
        }
        entry = {"B": B, "L": L, "L_resampled": Lo, "T": T, "steps": {}}
        for step, (run, nbytes) in steps.items():
            outs = {}
            for name, fn in run.items():                  # warm-up: code objects, rocFFT plans, cached tables
                for _ in range(3):
                    outs[name] = fn()
            torch.cuda.synchronize()
            ms = {name: [] for name in run}
            for _ in range(max(50, a.calls)):
                for name, fn in run.items():              # alternated: both legs see the same clocks and neighbours
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ms[name].append(e0.elapsed_time(e1))
            s = {"compulsory_bytes": nbytes,
                 "max_abs_diff_between_legs": float((outs["kernel"] - outs["torch"]).abs().max()), "max_abs": float(outs["torch"].abs().max())}
            for name, v in ms.items():
                q = statistics.quantiles(v, n=4)
                s[name + "_ms"] = {"median": statistics.median(v), "q1": q[0], "q3": q[2], "min": min(v), "max": max(v), "n": len(v)}
                s[name + "_launches_per_call"] = launches(run[name])
            s["torch_over_kernel"] = s["torch_ms"]["median"] / s["kernel_ms"]["median"]
            s["kernel_call_bytes_per_s"] = nbytes / (s["kernel_ms"]["median"] * 1e-3)
            entry["steps"][step] = s
            print(json.dumps({"B": B, "L": L, "step": step, **s}))
        result["sizes"].append(entry)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
