#!/usr/bin/env python
"""Timing of the speaker encoder: the HIP kernel path (csrc/spk.hip through the drop-in SpeakerEncoder) against torch.nn.LSTM + Linear
(the same module's torch path) on the same GPU, at U = 1 (a 10 s utterance: 12 partials of 160 frames), U = 16 (192 sequences) and one
sequence of 1000 frames.

  python tools/spk_prof.py [--calls 20] [--out profiles/spk_encoder.json]
      device events around every call, every shape warmed up, the two legs alternated call by call in one process; reports the
      median, the quartiles and the extremes per leg and their ratio (a ratio below 1 means the kernel path is slower: it is
      reported as it comes out).  The torch leg stacks the partials first, as the reference does.
  rocprofv3 --kernel-trace --stats -d DIR -o spk -- python tools/spk_prof.py --trace
      five calls per leg and shape, nothing else: the kernels' own times and the launch counts come from that run's trace;
  python tools/spk_prof.py --summarize DIR/..._kernel_trace.csv [--merge profiles/spk_encoder.json]
      per (shape, leg) launches per call and device time per call from the trace, merged into the JSON of the first form.
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
# (name, utterances, frames per utterance, partials, frame step, frames per partial)
SHAPES = (("U1_10s", 1, 1041, 12, 80, 160), ("U16_10s", 16, 1041, 12, 80, 160), ("N1_T1000", 1, 1000, 1, 0, 1000))
WARM, TRACE_CALLS = 2, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--merge", default=None)
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.merge)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("spk_prof.py needs a GPU")
    M = importlib.import_module("speech-backbones_amd.diffvc.speaker_encoder.encoder.model")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = M.SpeakerEncoder(dev, torch.device("cpu")).eval()
    result = {"calls": a.calls, "shapes": []}
    for name, U, T_total, P, S, T in SHAPES:
        frames = (0.01 * torch.rand(U, T_total, 40, generator=torch.Generator().manual_seed(U))).to(dev)

        def kernel():
            with torch.no_grad():
                return model.forward_partials(frames, P, S, T)[0]

        def torch_leg():
            with torch.no_grad():
                stacked = torch.stack([frames[u, p * S:p * S + T] for u in range(U) for p in range(P)], 0)
                out, (hidden, _) = model.lstm(stacked)
                raw = model.relu(model.linear(hidden[-1]))
                return raw / torch.norm(raw, dim=1, keepdim=True)
        run = {"kernel": kernel, "torch": torch_leg}
        outs = {}
        for leg, fn in run.items():                       # warm-up: code objects, MIOpen's choices, packed weights, workspace
            for _ in range(WARM):
                outs[leg] = fn()
        torch.cuda.synchronize()
        diff = float((outs["kernel"] - outs["torch"]).abs().max())
        if a.trace:
            for leg, fn in run.items():
                for _ in range(TRACE_CALLS):
                    fn()
                torch.cuda.synchronize()
            continue
        ms = {"kernel": [], "torch": []}
        for _ in range(max(8, a.calls)):
            for leg, fn in run.items():                   # alternated: both legs see the same clocks and neighbours
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[leg].append(e0.elapsed_time(e1))
        entry = {"shape": name, "U": U, "T_total": T_total, "P": P, "S": S, "T": T, "sequences": U * P, "max_abs_diff_between_legs": diff}
        for leg, v in ms.items():
            q = statistics.quantiles(v, n=4)
            entry[leg + "_ms"] = {"median": statistics.median(v), "q1": q[0], "q3": q[2], "min": min(v), "max": max(v), "n": len(v)}
        entry["torch_over_kernel"] = entry["torch_ms"]["median"] / entry["kernel_ms"]["median"]
        entry["kernel_us_per_step_and_layer"] = entry["kernel_ms"]["median"] * 1e3 / (3 * T)
        result["shapes"].append(entry)
        print(json.dumps(entry))
    if a.out and not a.trace:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


def summarize(path, merge):
    """The --trace run's kernel trace: per shape, in start order, WARM kernel-path calls, WARM torch calls, then TRACE_CALLS of each.
    A kernel-path call ends with its spk_utt_kernel; a timed call's span is everything after the previous call's end, so the
    drop-in's own torch launches (the parameter comparison that guards the packed weights) are counted with it."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    rows = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3) for r in rows]
    ends = [i for i, (n, _) in enumerate(rows) if "spk_utt_kernel" in n]
    firsts = [i for i, (n, _) in enumerate(rows) if "spk_proj_kernel" in n][::3]          # three layers per call
    per_shape = WARM + TRACE_CALLS
    out = []
    for s, shape in enumerate(SHAPES):
        e = ends[s * per_shape:(s + 1) * per_shape]
        calls = [(e[j - 1] + 1, e[j]) for j in range(WARM + 1, per_shape)]               # (the first timed call follows the torch warm-up)
        spans = [rows[i0:i1 + 1] for i0, i1 in calls]
        nxt = firsts[(s + 1) * per_shape] if (s + 1) * per_shape < len(firsts) else len(rows)
        torch_rows = [r for r in rows[calls[-1][1] + 1:nxt] if "spk_" not in r[0]]
        by_kernel = {}
        for sp in spans:
            for n, d in sp:
                k = n.split("(")[0].split("::")[-1][:40]
                by_kernel[k] = by_kernel.get(k, 0.0) + d / len(spans)
        out.append({"shape": shape[0], "kernel_launches_per_call": statistics.median(len(sp) for sp in spans),
                    "kernel_us_per_call": statistics.median(sum(d for _, d in sp) for sp in spans), "kernel_us_by_kernel": by_kernel,
                    "torch_launches_per_call": len(torch_rows) / TRACE_CALLS,
                    "torch_kernels_us_per_call": sum(d for _, d in torch_rows) / TRACE_CALLS,
                    "torch_kernels": sorted({n.split("(")[0][:80] for n, _ in torch_rows})[:24]})
        print(json.dumps(out[-1]))
    if merge:
        doc = json.load(open(merge))
        doc["kernel_trace"] = out
        with open(merge, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
