#!/usr/bin/env python
"""Timing of the log-mel front end: the HIP kernel path of hifi_gan/meldataset.py against the same module's torch recipe (pad, rocFFT
stft, magnitude, matmul, log) on the same GPU, at B = 16, L = 256 * 1024 (the bench's batch) and B = 1, L = 256 * 512 (one utterance).

  python tools/mel_prof.py [--calls 50] [--out mel_frontend.json]
      device events around every call, every shape warmed up, the two legs alternated call by call in one process; reports the
      median, the quartiles and the extremes per leg, their ratio, and the kernel path's bytes/s against the compulsory traffic
      4 B L + 4 B num_mels T (reported, no target: at these sizes the call is bound by launch latency).
  rocprofv3 --kernel-trace --stats -d DIR -o mel -- python tools/mel_prof.py --trace
      ten calls per leg and size, nothing else: the kernels' own times and the launch counts come from that run's trace;
  python tools/mel_prof.py --summarize DIR/..._kernel_trace.csv [--merge mel_frontend.json]
      per (size, leg) launches per call and device time per call from the trace, merged into the JSON of the first form.
A missing GPU is an error."""
import argparse
import csv
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CFG = (1024, 80, 22050, 256, 1024, 0, 8000)
SIZES = ((16, 256 * 1024), (1, 256 * 512))
TRACE_CALLS = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--merge", default=None)
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.merge)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mel_prof.py needs a GPU")
    MD = importlib.import_module("speech-backbones_amd.hifi_gan.meldataset")
    dev = torch.device("cuda:0")
    cfg = (CFG[0], CFG[1], CFG[2], CFG[3], CFG[4], float(CFG[5]), float(CFG[6]))
    result = {"config": list(CFG), "calls": a.calls, "sizes": []}
    for B, L in SIZES:
        y = (0.3 * torch.randn(B, L, generator=torch.Generator().manual_seed(B))).clamp(-1, 1).to(dev)
        run = {"kernel": lambda: MD.mel_spectrogram(y, *CFG), "torch": lambda: MD._torch_recipe(y, cfg, False)}
        outs = {}
        for name, fn in run.items():                      # warm-up: code objects, rocFFT plans, cached tables
            for _ in range(3):
                outs[name] = fn()
        torch.cuda.synchronize()
        diff = float((outs["kernel"] - outs["torch"]).abs().max())
        if a.trace:
            for name, fn in run.items():
                for _ in range(TRACE_CALLS):
                    fn()
                torch.cuda.synchronize()
            continue
        ms = {"kernel": [], "torch": []}
        for _ in range(max(20, a.calls)):
            for name, fn in run.items():                  # alternated: both legs see the same clocks and neighbours
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        T = outs["kernel"].shape[-1]
        entry = {"B": B, "L": L, "T": T, "max_abs_diff_between_legs": diff, "compulsory_bytes": 4 * B * L + 4 * B * CFG[1] * T}
        for name, v in ms.items():
            q = statistics.quantiles(v, n=4)
            entry[name + "_ms"] = {"median": statistics.median(v), "q1": q[0], "q3": q[2], "min": min(v), "max": max(v), "n": len(v)}
        entry["torch_over_kernel"] = entry["torch_ms"]["median"] / entry["kernel_ms"]["median"]
        entry["kernel_call_bytes_per_s"] = entry["compulsory_bytes"] / (entry["kernel_ms"]["median"] * 1e-3)
        result["sizes"].append(entry)
        print(json.dumps(entry))
    if a.out and not a.trace:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


def summarize(path, merge):
    """The --trace run's kernel trace: dispatches in order are, per size, 3 + 3 warm-up calls and then TRACE_CALLS calls of each leg;
    the mel kernel's dispatches separate the legs (one per kernel-path call)."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    rows = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3) for r in rows]
    is_mel = [i for i, (n, _) in enumerate(rows) if "mel_kernel" in n]
    per_size = 3 + TRACE_CALLS
    out = []
    for s, (B, L) in enumerate(SIZES):
        mel = is_mel[s * per_size:(s + 1) * per_size]
        timed = mel[3:]
        end = is_mel[(s + 1) * per_size] if (s + 1) * per_size < len(is_mel) else len(rows)
        torch_rows = rows[timed[-1] + 1:end]              # the timed torch calls follow the last timed kernel call of the size
        out.append({"B": B, "L": L, "kernel_launches_per_call": 1, "kernel_us": statistics.median(rows[i][1] for i in timed),
                    "torch_launches_per_call": len(torch_rows) / TRACE_CALLS,
                    "torch_kernels_us_per_call": sum(d for _, d in torch_rows) / TRACE_CALLS,
                    "torch_kernels": sorted({n.split("(")[0][:80] for n, _ in torch_rows})})
        print(json.dumps(out[-1]))
    if merge:
        doc = json.load(open(merge))
        doc["kernel_trace"] = out
        with open(merge, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
