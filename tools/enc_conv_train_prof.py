"""The encoders' Conv1d layers under autograd, forward + backward per layer kind, on the kernel path (_train_ops.EncConv1d: csrc/conv1d.h
data gradient, csrc/conv1d_train.hip weight gradient; the forward as wired -- torch's conv1d -- and with the inference kernel there too,
_train_ops.ENC_CONV_KERNEL_FORWARD) against torch.nn.Conv1d autograd (the path _train_ops.FORCE_TORCH selects: x * mask, the module call,
* mask), on the same GPU in the same process, the three alternated run by run.

Layer kinds (channels, kernel, which masks ride along, whether the input needs a gradient) are those of TextEncoder / MelEncoder at the
reference's widths; shapes are the two training shapes: B=16, L=190 (Grad-TTS train.py) and B=128, L=128 (DiffVC train_enc.py).  One run
is --inner forward + backward passes between two device events; medians of --reps runs (at least 9) with the quartiles after --warmup.
Prints one JSON object and writes it to --out (default profiles/enc_conv_train.json).

    python tools/enc_conv_train_prof.py [--reps 9] [--warmup 3] [--inner 10] [--out FILE]
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

SHAPES = (("gradtts_train", 16, 190), ("diffvc_train_enc", 128, 128))
# kind: (cin, cout, K, in_mask, out_mask, the input needs a gradient, where it occurs)
KINDS = {
    "prenet_k5": (192, 192, 5, True, False, True, "ConvReluNorm.conv_layers"),
    "proj_1x1": (192, 192, 1, False, False, True, "MultiHeadAttention.conv_q / k / v / o, ConvReluNorm.proj"),
    "ffn_1": (192, 768, 3, True, False, True, "FFN.conv_1"),
    "ffn_2": (768, 192, 3, True, True, True, "FFN.conv_2"),
    "proj_m": (192, 80, 1, False, True, True, "TextEncoder.proj_m, MelEncoder.term_proj"),
    "init_proj": (80, 192, 1, True, False, False, "MelEncoder.init_proj"),
    "dp_conv_1": (192, 256, 3, True, False, False, "DurationPredictor.conv_1 (detached input)"),
    "dp_conv_2": (256, 256, 3, True, False, True, "DurationPredictor.conv_2"),
    "dp_proj": (256, 1, 1, True, True, True, "DurationPredictor.proj"),
}


def _time(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def _alternate(TO, fn, reps, warm, inner):
    """(runs as wired, runs with the inference kernel in the forward too, torch runs) in ms per forward + backward, alternated run by run."""
    def with_flag(name, value):
        def leg():
            old = getattr(TO, name)
            setattr(TO, name, value)
            try:
                fn()
            finally:
                setattr(TO, name, old)
        return leg
    legs = [fn, with_flag("ENC_CONV_KERNEL_FORWARD", True), with_flag("FORCE_TORCH", True)]
    for _ in range(warm):
        for leg in legs:
            leg()
    torch.cuda.synchronize()
    runs = [[], [], []]
    for _ in range(reps):
        for k, leg in enumerate(legs):
            runs[k].append(_time(leg, inner))
    return runs


def _stats(v):
    q = statistics.quantiles(v, n=4)
    return {"median": round(statistics.median(v), 4), "q1": round(q[0], 4), "q3": round(q[2], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enc_conv_train.json"))
    args = ap.parse_args()
    assert args.reps >= 9, "medians of at least 9 runs"
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    TO = importlib.import_module("speech-backbones_amd.model._train_ops")
    TO.ENC_CONV_LEFT_ON_TORCH = frozenset()          # measure every kind on the kernels: this tool's numbers are what that set is decided from
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup, "inner": args.inner,
           "what": "ms per forward + backward of one Conv1d layer: EncConv1d as wired (torch forward, kernel backward), EncConv1d with the kernel forward, torch.nn.Conv1d autograd; alternated", "shapes": {}}
    for name, B, L in SHAPES:
        out = {"B": B, "L": L, "layers": {}}
        lens = torch.linspace(L, max(1, L // 3), B).round().long()
        mask = (torch.arange(L)[None] < lens[:, None]).float().unsqueeze(1).to(dev)
        for kind, (cin, cout, K, im, om, xg, where) in KINDS.items():
            torch.manual_seed(0)
            g = torch.Generator().manual_seed(1)
            conv = torch.nn.Conv1d(cin, cout, K, padding=K // 2).to(dev)
            x = torch.randn(B, cin, L, generator=g).to(dev).requires_grad_(xg)
            dy = torch.randn(B, cout, L, generator=g).to(dev)

            def layer():
                x.grad = conv.weight.grad = conv.bias.grad = None
                TO.enc_conv1d(conv, x, in_mask=mask if im else None, out_mask=mask if om else None).backward(dy)

            TO.reset_enc_conv_op_counts()
            layer()
            assert TO.enc_conv_op_counts() == (1, 0), "the kernel path did not run: %s" % (TO.enc_conv_op_counts(),)
            hip, hipf, ref = _alternate(TO, layer, args.reps, args.warmup, args.inner)
            out["layers"][kind] = {"cin": cin, "cout": cout, "K": K, "in_mask": im, "out_mask": om, "input_grad": xg, "where": where,
                                   "hip_ms": _stats(hip), "hip_kernel_forward_ms": _stats(hipf), "torch_ms": _stats(ref),
                                   "speedup": round(statistics.median(ref) / statistics.median(hip), 3),
                                   "speedup_kernel_forward": round(statistics.median(ref) / statistics.median(hipf), 3)}
        res["shapes"][name] = out
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
