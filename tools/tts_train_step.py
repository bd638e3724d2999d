"""One Grad-TTS training step with the encoder attached -- GradTTS.compute_loss forward + backward as Grad-TTS/train.py:95-110 drives it -- at
the reference's shape: B = 16, out_size = 172 frames (2 s), x_lengths 60 ... 190 tokens, y_lengths 300 ... 860 frames, model.train().  In
one process it times the kernel path and, with _train_ops.FORCE_TORCH, the same step on stock PyTorch-ROCm ops; it reports the median of
`--reps` steps after `--warmup` for each, and the op counters of one kernel-path step.  Only public calls are used, so the same file runs
on an older checkout (counters it does not have are reported as null).  Prints one JSON object (and writes it to --out).

    python tools/tts_train_step.py [--B 16] [--out-size 172] [--warmup 3] [--reps 7] [--out FILE]

profiles/tts_train_step.json holds such runs of this tree and of its parent commit, alternated in one GPU visit."""
import argparse
import importlib
import json
import os
import random
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--out-size", type=int, default=172)
    ap.add_argument("--n-spks", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert args.reps >= 5, "the median of at least 5 steps"
    dev = torch.device("cuda:0")
    M = importlib.import_module("speech-backbones_amd.model")
    TO = importlib.import_module("speech-backbones_amd.model._train_ops")
    torch.manual_seed(0)
    model = M.GradTTS(149, args.n_spks, 64, 192, 768, 256, 2, 6, 3, 0.1, 4, 80, 64, 0.05, 20.0, 1000).to(dev).train()
    g = torch.Generator().manual_seed(1)
    B = args.B
    x_lengths = torch.linspace(190, 60, B).round().long()
    y_lengths = torch.linspace(860, 300, B).round().long()
    tx, T = int(x_lengths.max()), (int(y_lengths.max()) + 3) // 4 * 4
    x = (torch.randint(0, 149, (B, tx), generator=g) * (torch.arange(tx)[None] < x_lengths[:, None])).to(dev)
    y = (torch.randn(B, 80, T, generator=g) * (torch.arange(T)[None, None] < y_lengths[:, None, None])).to(dev)
    spk = torch.randint(0, args.n_spks, (B,), generator=g).to(dev) if args.n_spks > 1 else None
    x_lengths, y_lengths = x_lengths.to(dev), y_lengths.to(dev)

    def step():
        model.zero_grad(set_to_none=True)
        sum(model.compute_loss(x, x_lengths, y, y_lengths, spk=spk, out_size=args.out_size)).backward()

    res = {"workload": "GradTTS.compute_loss forward + backward (Grad-TTS/train.py), %d speaker(s), B=%d, out_size=%d, x_lengths %d..%d, "
                       "y_lengths %d..%d, train() mode" % (args.n_spks, B, args.out_size, int(x_lengths.min()), tx, int(y_lengths.min()),
                                                           int(y_lengths.max())),
           "device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup}
    counters = {"decoder": ("reset_op_counts", "op_counts"), "encoder": ("reset_enc_op_counts", "enc_op_counts"),
                "glue": ("reset_glue_op_counts", "glue_op_counts"), "encoder_conv": ("reset_enc_conv_op_counts", "enc_conv_op_counts")}
    for reset, _ in counters.values():
        getattr(TO, reset, lambda: None)()
    random.seed(0)
    step()
    torch.cuda.synchronize()
    for name, (_, read) in counters.items():
        res["%s_ops_hip_fallback" % name] = list(getattr(TO, read)()) if hasattr(TO, read) else None
    random.seed(0)
    ms, all_ms = _median_ms(step, args.reps, args.warmup)
    res["hip_ms"], res["hip_ms_runs"] = round(ms, 3), [round(t, 3) for t in all_ms]
    TO.FORCE_TORCH = True
    try:
        random.seed(0)
        ms, all_ms = _median_ms(step, args.reps, args.warmup)
    finally:
        TO.FORCE_TORCH = False
    res["torch_rocm_ms"], res["torch_rocm_ms_runs"] = round(ms, 3), [round(t, 3) for t in all_ms]
    res["speedup"] = round(res["torch_rocm_ms"] / res["hip_ms"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
