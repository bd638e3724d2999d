"""One GE2E training step of the DiffVC speaker encoder (DiffVC/speaker_encoder/encoder/train.py:92-108: forward, loss, backward,
do_gradient_ops, Adam) at the reference's shape -- 64 speakers x 10 utterances of 160 frames (encoder/params_model.py) -- through
encoder.ge2e.SpeakerEncoder on the HIP kernels (csrc/spk_train.hip) and, in the same process and alternated with it, on stock
PyTorch-ROCm: torch.nn.LSTM autograd with the vectorised torch loss on the same GPU.  Also times the loss alone: the GE2E kernel
(similarity matrix, loss and all three gradients in one launch) against the reference's arrangement -- embeddings copied to the CPU, the
similarity matrix filled by a Python loop over the speakers, cross-entropy and backward there.  Prints one JSON object (and writes it to
--out).

    python tools/spk_train_step.py [--S 64] [--U 10] [--T 160] [--warmup 2] [--reps 5] [--out profiles/spk_train_step.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _loop_loss_cpu(embeds, w, b):
    """model.py:65-126 of the reference on CPU tensors, its loop over the speakers included (plain ints for np.int)."""
    S, U = embeds.shape[:2]
    incl = torch.mean(embeds, dim=1, keepdim=True)
    incl = incl.clone() / torch.norm(incl, dim=2, keepdim=True)
    excl = (torch.sum(embeds, dim=1, keepdim=True) - embeds) / (U - 1)
    excl = excl.clone() / torch.norm(excl, dim=2, keepdim=True)
    sim = torch.zeros(S, U, S)
    for j in range(S):
        mask = [s for s in range(S) if s != j]
        sim[mask, :, j] = (embeds[mask] * incl[j]).sum(dim=2)
        sim[j, :, j] = (embeds[j] * excl[j]).sum(dim=1)
    sim = sim * w + b
    return torch.nn.functional.cross_entropy(sim.reshape(S * U, S), torch.arange(S).repeat_interleave(U))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=64)
    ap.add_argument("--U", type=int, default=10)
    ap.add_argument("--T", type=int, default=160)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    L = importlib.import_module("speech-backbones_amd")
    G = importlib.import_module("speech-backbones_amd.diffvc.speaker_encoder.encoder.ge2e")
    S, U, T = args.S, args.U, args.T
    torch.manual_seed(0)
    hip = G.SpeakerEncoder(dev, dev)
    stock = G.SpeakerEncoder(dev, dev)
    stock.load_state_dict(hip.state_dict())
    stock._train_kernel_ok = lambda *a: False          # torch.nn.LSTM autograd
    stock._ge2e_kernel_ok = lambda *a: False           # the vectorised torch loss
    x = 0.5 * torch.randn(S * U, T, 40, generator=torch.Generator().manual_seed(1)).to(dev)

    def make_step(model):
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)
        out = {}

        def step():
            model.zero_grad()
            embeds = model(x)
            loss, _ = model.loss(embeds.view(S, U, -1), want_eer=False)
            loss.backward()
            model.do_gradient_ops()
            opt.step()
            out["loss"] = loss.detach()
        return step, out

    steps = {"hip": make_step(hip), "stock": make_step(stock)}
    times = {"hip": [], "stock": []}
    first_loss = {}
    for k in range(args.warmup + args.reps):
        for name in ("hip", "stock"):
            ms = _timed_ms(steps[name][0])
            if k == 0:
                first_loss[name] = float(steps[name][1]["loss"])
            if k >= args.warmup:
                times[name].append(ms)
    # the parts of the HIP step
    plan, blob, blob_train = hip._packed_train(dev)
    d = torch.randn(S * U, 256, device=dev)
    parts = {"forward_train": [], "backward": []}
    for k in range(args.warmup + args.reps):
        box = {}
        f = _timed_ms(lambda: box.update(out=plan.forward_train(blob, x)))
        b = _timed_ms(lambda: plan.backward(blob_train, x, d, box["out"][1]))
        if k >= args.warmup:
            parts["forward_train"].append(f)
            parts["backward"].append(b)
    # the loss alone
    with torch.no_grad():
        embeds = hip(x).view(S, U, -1).contiguous()
    w, b = hip.similarity_weight.detach(), hip.similarity_bias.detach()
    loss_hip, loss_cpu = [], []
    for k in range(args.warmup + args.reps):
        ms = _timed_ms(lambda: L.ge2e_loss(embeds, w, b))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e_cpu = embeds.cpu().requires_grad_(True)
        wc, bc = w.cpu().requires_grad_(True), b.cpu().requires_grad_(True)
        _loop_loss_cpu(e_cpu, wc, bc).backward()
        e_cpu.grad.to(dev)
        torch.cuda.synchronize()
        cpu_ms = (time.perf_counter() - t0) * 1e3
        if k >= args.warmup:
            loss_hip.append(ms)
            loss_cpu.append(cpu_ms)
    med = statistics.median
    res = {
        "shape": {"speakers": S, "utterances": U, "frames": T},
        "device": torch.cuda.get_device_name(0),
        "step_ms": {"hip": med(times["hip"]), "stock": med(times["stock"]), "hip_all": times["hip"], "stock_all": times["stock"]},
        "hip_parts_ms": {k: med(v) for k, v in parts.items()},
        "first_step_loss": first_loss,
        "loss_alone_ms": {"hip_kernel": med(loss_hip), "cpu_copy_and_loop": med(loss_cpu)},
        "saved_state_bytes": plan.saved_bytes(S * U, T),
        "warmup": args.warmup, "reps": args.reps,
    }
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
