"""Checker of the speaker encoder's training path (csrc/spk_train.hip, diffvc/speaker_encoder/encoder/ge2e.py): float64 restatements on
the CPU with autograd gradients, seeded fixtures, and for each the same recipe in float32 torch on the CPU (`e_ref32`).

  embeddings(kind, S, U)            [S, U, 256] float32: 'model' = rows of relu(randn), normalised; 'clustered' = a speaker mean (uniform in
                                    [0, 1): with randn means the softmax saturates and the reference's own float32 gradients are 4e-5
                                    off) plus 0.1 randn noise, through relu, normalised
  ge2e(embeds, w, b, dtype)         the reference's similarity matrix WITH its loop over speakers (plain ints), cross-entropy, autograd
  ge2e_reference(kind, S, U)        float64 results and per-tensor e_ref32
  encoder_backward(...)             nn.LSTM + head in `dtype`, e.backward(d) for the upstream d = upstream(N)
  encoder_reference(...)            float64 gradients, per-tensor e_ref32, the float64 pre-ReLU values
  step_reference(S, U, T, mask)     model(x) -> loss -> backward on 'trained' weights and 'noise' frames: all 16 gradients
Weights and frames come from spk_oracle.  ReLU mask: a [N, 256] bool tensor replaces relu(pre) by pre * mask in both precisions, so that
a unit whose float64 pre-activation lies within rounding of zero is taken the way the run under test took it (one flipped unit moves a
gradient by percent).  Errors are per tensor: err(got, g64) = max |got - g64| / max |g64|.  Results are cached: do not modify."""
import functools

import torch

import spk_oracle as SO

KINDS = ("model", "clustered")
W0, B0 = 10.0, -5.0
PARAMS = [n for l in range(SO.LAYERS) for n in ("lstm.weight_ih_l%d" % l, "lstm.weight_hh_l%d" % l, "lstm.bias_ih_l%d" % l,
                                                "lstm.bias_hh_l%d" % l)] + ["linear.weight", "linear.bias"]


def err(got, g64):
    got, g64 = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(g64).double().reshape(-1)
    return float((got - g64).abs().max() / g64.abs().max())


@functools.lru_cache(maxsize=None)
def embeddings(kind, S, U):
    g = torch.Generator().manual_seed(77000 + 1000 * KINDS.index(kind) + 31 * S + U)
    if kind == "model":
        e = torch.relu(torch.randn(S, U, SO.EMBED, generator=g))
    else:
        mean = torch.rand(S, 1, SO.EMBED, generator=g)          # non-negative like a ReLU output: speakers stay within reach of each other
        e = torch.relu(mean + 0.1 * torch.randn(S, U, SO.EMBED, generator=g))
    return e / torch.norm(e, dim=2, keepdim=True)


def checksum(e):
    """float64: position-weighted sum of a fixture, to tell a regenerated input from the recorded one."""
    e = e.double().reshape(-1)
    return float((e * torch.linspace(1.0, 2.0, e.numel(), dtype=torch.float64)).sum())


def similarity(embeds, w, b):
    S, U = embeds.shape[:2]
    incl = torch.mean(embeds, dim=1, keepdim=True)
    incl = incl / torch.norm(incl, dim=2, keepdim=True)
    excl = (torch.sum(embeds, dim=1, keepdim=True) - embeds) / (U - 1)
    excl = excl / torch.norm(excl, dim=2, keepdim=True)
    cols = []
    for j in range(S):
        col = (embeds * incl[j]).sum(dim=2)                       # [S, U]
        own = (embeds[j] * excl[j]).sum(dim=1)                    # [U]
        rows = [own if s == j else col[s] for s in range(S)]
        cols.append(torch.stack(rows))
    return torch.stack(cols, dim=2) * w + b


def ge2e(embeds, w, b, dtype):
    """-> dict(sim [S U, S], loss, d_embeds, dw, db) in `dtype`."""
    e = embeds.to(dtype).clone().requires_grad_(True)
    w = torch.tensor([w], dtype=dtype, requires_grad=True)
    b = torch.tensor([b], dtype=dtype, requires_grad=True)
    S, U = e.shape[:2]
    sim = similarity(e, w, b).reshape(S * U, S)
    target = torch.arange(S).repeat_interleave(U)
    loss = torch.nn.functional.cross_entropy(sim, target)
    loss.backward()
    return dict(sim=sim.detach(), loss=loss.detach().reshape(1), d_embeds=e.grad, dw=w.grad, db=b.grad)


@functools.lru_cache(maxsize=None)
def ge2e_reference(kind, S, U):
    """(g64, e_ref32): float64 results, and per tensor the normalised error of the float32 run (db: absolute)."""
    e = embeddings(kind, S, U)
    g64, g32 = ge2e(e, W0, B0, torch.float64), ge2e(e, W0, B0, torch.float32)
    e32 = {k: (float((g32[k].double() - g64[k]).abs().max()) if k == "db" else err(g32[k], g64[k])) for k in g64}
    return g64, e32


# ---- encoder
@functools.lru_cache(maxsize=None)
def upstream(N):
    return torch.randn(N, SO.EMBED, generator=torch.Generator().manual_seed(4100 + N))


def _encoder(sd, dtype):
    lstm, lin = SO._modules(dtype)
    lstm.load_state_dict({k[5:]: v.to(dtype) for k, v in sd.items() if k.startswith("lstm.")})
    lin.load_state_dict({k[7:]: v.to(dtype) for k, v in sd.items() if k.startswith("linear.")})
    return lstm, lin


def _embed(lstm, lin, x, mask):
    _, (h, _) = lstm(x)
    pre = lin(h[-1])
    raw = torch.relu(pre) if mask is None else pre * mask.to(pre.dtype)
    return pre, raw / torch.norm(raw, dim=1, keepdim=True)


def _grads(lstm, lin):
    out = {"lstm." + k: p.grad for k, p in lstm.named_parameters()}
    out.update({"linear." + k: p.grad for k, p in lin.named_parameters()})
    return out


def encoder_backward(weights, inputs, N, T, dtype, mask=None):
    """-> (gradients by parameter name, pre-ReLU [N, 256], embeds) in `dtype`."""
    lstm, lin = _encoder(SO.state(weights), dtype)
    pre, e = _embed(lstm, lin, SO.frames(inputs, N, T).to(dtype), mask)
    e.backward(upstream(N).to(dtype))
    return _grads(lstm, lin), pre.detach(), e.detach()


_ENC = {}


def _mask_key(mask):
    return None if mask is None else bytes(mask.to(torch.uint8).reshape(-1).tolist())


def encoder_reference(weights, inputs, N, T, mask=None):
    """(g64 by name, e_ref32 by name, pre64).  mask None: float64's own relu (and the float32 run takes float64's mask, so that e_ref32
    measures rounding and not a unit that float32 flipped)."""
    if mask is not None:
        own = encoder_reference(weights, inputs, N, T)
        if torch.equal(mask.cpu(), own[2] > 0):
            return own
    key = (weights, inputs, N, T, _mask_key(mask))
    if key not in _ENC:
        if mask is None:
            _, pre64, _ = encoder_backward(weights, inputs, N, T, torch.float64)
            mask = pre64 > 0
        g64, pre64, _ = encoder_backward(weights, inputs, N, T, torch.float64, mask)
        g32, _, _ = encoder_backward(weights, inputs, N, T, torch.float32, mask)
        _ENC[key] = (g64, {k: err(g32[k], g64[k]) for k in g64}, pre64)
    return _ENC[key]


# ---- the whole step
def step(S, U, T, dtype, mask=None):
    lstm, lin = _encoder(SO.state("trained"), dtype)
    w = torch.tensor([W0], dtype=dtype, requires_grad=True)
    b = torch.tensor([B0], dtype=dtype, requires_grad=True)
    pre, e = _embed(lstm, lin, SO.frames("noise", S * U, T).to(dtype), mask)
    sim = similarity(e.view(S, U, -1), w, b).reshape(S * U, S)
    loss = torch.nn.functional.cross_entropy(sim, torch.arange(S).repeat_interleave(U))
    loss.backward()
    g = _grads(lstm, lin)
    g.update(similarity_weight=w.grad, similarity_bias=b.grad)
    return g, pre.detach(), loss.detach()


_STEP = {}


def step_reference(S, U, T, mask=None):
    """(g64 by name, e_ref32 by name, pre64, loss64); similarity_bias: absolute error, its gradient is analytically zero."""
    if mask is not None:
        own = step_reference(S, U, T)
        if torch.equal(mask.cpu(), own[2] > 0):
            return own
    key = (S, U, T, _mask_key(mask))
    if key not in _STEP:
        if mask is None:
            mask = step(S, U, T, torch.float64)[1] > 0
        g64, pre64, loss64 = step(S, U, T, torch.float64, mask)
        g32 = step(S, U, T, torch.float32, mask)[0]
        e32 = {k: (float((g32[k].double() - g64[k]).abs().max()) if k == "similarity_bias" else err(g32[k], g64[k])) for k in g64}
        _STEP[key] = (g64, e32, pre64, loss64)
    return _STEP[key]


def near_zero(pre64, tol=1e-5):
    return pre64.abs() <= tol


# ---- the cases of the GPU tests (tests/test_gpu_spk_train.py); tests/test_ge2e_cpu.py proves the fixture conditions for each
GE2E_SHAPES = [(2, 2), (3, 4), (5, 3), (8, 5), (64, 10)]
ENC_SHAPES = [(1, 1), (1, 2), (3, 7), (16, 160), (17, 160), (20, 33), (40, 160), (1, 257), (2, 129)]
STEP_SHAPES = [(2, 2, 1), (3, 4, 7), (2, 8, 160), (3, 6, 160), (8, 5, 160)]
