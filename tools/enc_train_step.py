"""One DiffVC "average voice" encoder training step (FwdDiffusion.compute_loss forward + backward, DiffVC/model/vc.py:43-48, as
DiffVC/train_enc.py:83-91 drives it) at the reference's shape -- channels 192, filters 768, heads 2, layers 6, window 4, enc_dim 128,
B = 128 of 128-frame crops (DiffVC/params.py, train_enc.py:45) -- with the PostNet on the gtts:: training kernels and, in the same
process, with every op on stock PyTorch-ROCm (_train_ops.FORCE_TORCH).  Also times the 7x7 weight-gradient kernel alone at the
PostNet Block's shape.  Prints one JSON object (and writes it to --out).

    python tools/enc_train_step.py [--B 128] [--T 128] [--warmup 2] [--reps 5] [--out FILE]
"""
import argparse
import importlib
import json
import os
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
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    S = importlib.import_module("speech-backbones_amd")
    VC = importlib.import_module("speech-backbones_amd.diffvc.model.vc")
    TO = importlib.import_module("speech-backbones_amd.model._train_ops")
    torch.manual_seed(0)
    enc = VC.FwdDiffusion(80, 192, 768, 2, 6, 3, 0.1, 4, args.dim).to(dev).train()
    g = torch.Generator().manual_seed(1)
    B, T = args.B, args.T
    x = torch.randn(B, 80, T, generator=g).to(dev)
    y = torch.randn(B, 80, T, generator=g).to(dev)
    mask = torch.ones(B, 1, T, device=dev)

    def step():
        enc.zero_grad(set_to_none=True)
        enc.compute_loss(x, y, mask).backward()

    res = {"workload": "DiffVC FwdDiffusion.compute_loss forward + backward (DiffVC/train_enc.py:83-91), channels 192, filters 768, "
                       "heads 2, layers 6, window 4, enc_dim %d, B=%d x 80x%d, train() mode" % (args.dim, B, T),
           "device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup}
    TO.reset_op_counts()
    step()
    res["hip_ops"], res["torch_fallback_ops"] = TO.op_counts()
    ms, all_ms = _median_ms(step, args.reps, args.warmup)
    res["hip_ms"], res["hip_ms_runs"] = round(ms, 3), [round(t, 3) for t in all_ms]
    TO.FORCE_TORCH = True
    try:
        ms, all_ms = _median_ms(step, args.reps, args.warmup)
    finally:
        TO.FORCE_TORCH = False
    res["torch_rocm_ms"], res["torch_rocm_ms_runs"] = round(ms, 3), [round(t, 3) for t in all_ms]
    res["speedup"] = round(res["torch_rocm_ms"] / res["hip_ms"], 3)
    # the 7x7 weight gradient alone at the Block's shape: 49 x C^2 x B x 80 x T MACs, 3 bf16 MFMAs per product (split-bf16)
    C = args.dim
    xa = torch.randn(B, C, 80, T, device=dev)
    dy = torch.randn(B, C, 80, T, device=dev)
    cols = mask.reshape(B, T).contiguous()
    ms, _ = _median_ms(lambda: S._lib.conv7x7_wgrad(xa, cols, dy), args.reps, args.warmup)
    executed = 3 * 2.0 * 49 * C * C * B * 80 * T
    res["wgrad7_ms"] = round(ms, 3)
    res["wgrad7_executed_tflop"] = round(executed / 1e12, 3)
    res["wgrad7_spec_ceiling_ms"] = round(executed / 2.5e15 * 1e3, 3)     # 2.5 PF dense bf16 (spec), derived, not measured
    res["wgrad7_vs_ceiling"] = round(ms / res["wgrad7_spec_ceiling_ms"], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
