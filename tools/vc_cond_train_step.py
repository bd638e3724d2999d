"""One DiffVC decoder training step -- Diffusion.compute_loss forward + backward as DiffVC/train_dec.py:90-103 drives it -- at that script's
shape: dim_unet 256, dim_spk 128, use_ref_t, B = 16, 128-frame crops.  Reports the median of `--reps` steps after `--warmup` (device
events), the peak allocated memory of a step, and the op counters.  Only public calls are used, so the same file runs on an older checkout
(counters it does not have are reported as null).  With --layers it also times, per narrow RefBlock layer kind and for the two condition
fields, the kernels of this tree against the stock ops they replace (forward + every gradient, at the step's shapes).  Prints one JSON
object (and writes it to --out).

    python tools/vc_cond_train_step.py [--B 16] [--T 128] [--warmup 3] [--reps 9] [--layers] [--out FILE]

profiles/vc_cond_train.json holds such runs of this tree and of its parent commit, alternated in one GPU visit."""
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


def _layers(TO, L, dev, B, T, reps, warm):
    """{layer: {hip_ms, torch_ms}}: forward + weight / bias gradient (+ data gradient where the step takes one) per call."""
    F = torch.nn.functional
    g = torch.Generator().manual_seed(2)
    mask = torch.ones(B, 1, 1, T, device=dev)
    out = {}
    for name, cin, cout, need_dx in (("block11 1->64", 1, 64, False), ("block12 32->64", 32, 64, True), ("block21 32->128", 32, 128, True)):
        x = torch.randn(B, cin, 80, T, generator=g).to(dev).requires_grad_(need_dx)
        w = (torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5)).to(dev).requires_grad_(True)
        b = torch.zeros(cout, device=dev, requires_grad=True)
        dy = torch.randn(B, cout, 80, T, generator=g).to(dev)

        def run(hip):
            for v in (x, w, b):
                v.grad = None
            y = TO.MaskedConv3x3.apply(x, mask, w, b, None) if hip else F.conv2d(x * mask, w, b, padding=1)
            y.backward(dy)
        out[name] = {"hip_ms": _median_ms(lambda: run(True), reps, warm)[0], "torch_ms": _median_ms(lambda: run(False), reps, warm)[0]}
    # the condition columns of the first ResnetBlock: the field against the convolution of the broadcast plane on stock ops
    for name, k in (("cond columns 3x3 128->256", 3), ("cond columns 1x1 128->256", 1)):
        cond = torch.randn(B, 128, generator=g).to(dev).requires_grad_(True)
        w = (torch.randn(256, 128, k, k, generator=g) / (k * 128 ** 0.5)).to(dev).requires_grad_(True)
        base = torch.randn(B, 256, 80, T, generator=g).to(dev)
        dy = torch.randn(B, 256, 80, T, generator=g).to(dev)

        def run(hip):
            cond.grad = w.grad = None
            if hip:
                u = torch.einsum("ocij,bc->bijo", w, cond).reshape(B, k * k, 256)
                y = TO.CondField.apply(u.contiguous(), mask, base)
            else:
                y = base + F.conv2d(cond[:, :, None, None].expand(-1, -1, 80, T) * mask, w, None, padding=k // 2)
            y.backward(dy)
        out[name] = {"hip_ms": _median_ms(lambda: run(True), reps, warm)[0], "torch_ms": _median_ms(lambda: run(False), reps, warm)[0]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert args.reps >= 5, "the median of at least 5 steps"
    dev = torch.device("cuda:0")
    DV = importlib.import_module("speech-backbones_amd.diffvc.model.diffusion")
    TO = importlib.import_module("speech-backbones_amd.model._train_ops")
    L = importlib.import_module("speech-backbones_amd")._lib
    torch.manual_seed(0)
    dec = DV.Diffusion(80, 256, 128, True, 0.05, 20.0).to(dev)
    g = torch.Generator().manual_seed(1)
    B, T = args.B, args.T
    x0, mean, xr, mr = (torch.randn(B, 80, T, generator=g).to(dev) for _ in range(4))
    c = (torch.randn(B, 256, generator=g) * 0.3).to(dev)
    mask = torch.ones(B, 1, T, device=dev)

    def step():
        dec.zero_grad(set_to_none=True)
        dec.compute_loss(x0, mask, mean, xr, mr, c).backward()

    res = {"workload": "DiffVC Diffusion.compute_loss forward + backward (DiffVC/train_dec.py), dim_unet 256, dim_spk 128, use_ref_t, "
                       "B=%d, T=%d" % (B, T), "device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup}
    counters = {"decoder": ("reset_op_counts", "op_counts"), "condition": ("reset_cond_op_counts", "cond_op_counts")}
    for reset, _ in counters.values():
        getattr(TO, reset, lambda: None)()
    step()
    torch.cuda.synchronize()
    res["op_counts"] = {name: (list(getattr(TO, read)()) if hasattr(TO, read) else None) for name, (_, read) in counters.items()}
    left = getattr(TO, "COND_LEFT_ON_TORCH", None)
    res["cond_left_on_torch"] = None if left is None else sorted(list(k) for k in left)
    med, times = _median_ms(step, args.reps, args.warmup)
    res["step_ms"], res["step_ms_all"] = med, times
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    step()
    torch.cuda.synchronize()
    res["peak_allocated_mib"] = torch.cuda.max_memory_allocated(dev) / 2 ** 20
    res["allocated_before_step_mib"] = base / 2 ** 20
    if args.layers:
        res["layers"] = _layers(TO, L, dev, B, T, args.reps, args.warmup)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
