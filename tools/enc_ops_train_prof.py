"""The encoders' two kernel ops under autograd, forward + backward, on the kernels of csrc/enc_train.hip against the module's own torch
composition (the path _train_ops.FORCE_TORCH selects), on the same GPU in the same process, the two alternated run by run:

  attention   MultiHeadAttention.attention between its convolutions (q, k, v -> out, then out.backward): relative window 4, dropout 0.1
  layernorm   LayerNorm(x, bres) forward + backward (the fused residual form Encoder.forward calls)

at the reference's two training shapes: B=16, C=192, H=2, L=180 (Grad-TTS train.py) and B=128, L=128 (DiffVC train_enc.py).  Medians of
--reps runs (at least 5) after --warmup; prints one JSON object and writes it to --out (default profiles/enc_train_ops.json).

    python tools/enc_ops_train_prof.py [--reps 9] [--warmup 3] [--out FILE]
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

SHAPES = (("gradtts_train", 16, 192, 2, 180), ("diffvc_train_enc", 128, 192, 2, 128))


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _alternate(TO, fn, reps, warm):
    """(kernel-path runs, composition runs) in ms, alternated: kernel, composition, kernel, ..."""
    def torch_path():
        TO.FORCE_TORCH = True
        try:
            fn()
        finally:
            TO.FORCE_TORCH = False
    for _ in range(warm):
        fn()
        torch_path()
    torch.cuda.synchronize()
    hip, ref = [], []
    for _ in range(reps):
        hip.append(_time(fn))
        ref.append(_time(torch_path))
    return hip, ref


def _entry(hip, ref):
    r = lambda v: [round(t, 4) for t in v]
    return {"hip_ms": round(statistics.median(hip), 4), "torch_ms": round(statistics.median(ref), 4), "hip_ms_runs": r(hip), "torch_ms_runs": r(ref),
            "speedup": round(statistics.median(ref) / statistics.median(hip), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enc_train_ops.json"))
    args = ap.parse_args()
    assert args.reps >= 5, "a median of at least 5 runs"
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    TE = importlib.import_module("speech-backbones_amd.model.text_encoder")
    TO = importlib.import_module("speech-backbones_amd.model._train_ops")
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup,
           "what": "forward + backward per op, kernel path (csrc/enc_train.hip) vs the module's torch composition, alternated", "shapes": {}}
    for name, B, C, H, L in SHAPES:
        torch.manual_seed(0)
        g = torch.Generator().manual_seed(1)
        att = TE.MultiHeadAttention(C, C, H, window_size=4, p_dropout=0.1).to(dev).train()
        q, k, v = (torch.randn(B, C, L, generator=g).to(dev).requires_grad_(True) for _ in range(3))
        dout = torch.randn(B, C, L, generator=g).to(dev)
        seq = torch.ones(B, 1, L, device=dev)
        pair = seq.unsqueeze(2) * seq.unsqueeze(-1)

        def attention():
            for t in (q, k, v, att.emb_rel_k, att.emb_rel_v):
                t.grad = None
            out, _ = att.attention(q, k, v, mask=pair, seq_mask=seq, self_attention=True)
            out.backward(dout)

        ln = TE.LayerNorm(C).to(dev)
        x, y = (torch.randn(B, C, L, generator=g).to(dev).requires_grad_(True) for _ in range(2))

        def layernorm():
            for t in (x, y, ln.gamma, ln.beta):
                t.grad = None
            ln(x, y).backward(dout)

        TO.reset_enc_op_counts()
        attention()
        layernorm()
        assert TO.enc_op_counts() == (2, 0), "the kernel path did not run: %s" % (TO.enc_op_counts(),)
        res["shapes"][name] = {"B": B, "C": C, "H": H, "L": L, "attention": _entry(*_alternate(TO, attention, args.reps, args.warmup)),
                               "layernorm": _entry(*_alternate(TO, layernorm, args.reps, args.warmup))}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
