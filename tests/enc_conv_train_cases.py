"""Catalogue of single-layer cases of the encoders' Conv1d training path -- EncConv1d (model/_train_ops.py): forward and data gradient on
the inference kernel (csrc/conv1d.h), weight / bias gradient on csrc/conv1d_train.hip -- with their float64 reference and the formulas
of include/gradtts_abi.h restated in torch.

    y  = (conv1d(x * im, W, dilation) + bias) * om                          off(t) = (t - (K - 1) / 2) * dilation
    dx = conv1d(dy * om, W', dilation) * im,   W'[ci][co][t] = W[co][ci][K - 1 - t]
    dw[co][ci][t] = sum_b sum_q (dy * om)[b, co, q] * (x * im)[b, ci, q + off(t)]     (zero where q + off(t) leaves [0, L))
    db[co] = sum_b sum_q (dy * om)[b, co, q]

tests/test_gpu_enc_conv_train_ops.py runs every case on the GPU; tests/test_enc_conv_train_cases_cpu.py proves without one that the
catalogue reaches every regime of the weight-gradient launcher it claims (Conv1dOp.wgrad_info: the launcher's own arithmetic), that the
formulas equal float64 autograd, and that the bound tells seven restated mistakes from the kernels.

Shapes are the smallest at which each geometry can still go wrong: the encoders' real widths at B = 2 and L <= 70, everything else on
a few channels; B >= 2 wherever a read across a sample boundary could show."""
import collections

import torch
import torch.nn.functional as F

from case_util import relerr, seq_mask  # noqa: F401

REL = 1e-4          # split-bf16 contractions, fp32 accumulate: e = max |got - ref| / max |ref| per tensor (tests/conv1d_cases.py)
CHUNK = 64          # positions per chunk of the weight-gradient kernel (checked against wgrad_info by the CPU test)
TILE = 64           # its output tile, rows (co) and columns (ci)


def db_bound(e_ref32):
    """db is a plain fp32 sum: four times the error of the same sum in fp32 torch, plus 2e-6 for sums that fp32 torch gets exactly."""
    return 4.0 * e_ref32 + 2e-6


Case = collections.namedtuple("Case", "id cin cout K dil B L in_lens out_lens bias x_grad")


def case(id, cin, cout, K, L, dil=1, B=2, in_lens=None, out_lens=None, bias=True, x_grad=True):
    return Case(id, cin, cout, K, dil, B, L, in_lens, out_lens, bias, x_grad)


def _cases():
    c = []
    # ---- the shape of the encoder module tests: widths 24 / 48, ragged lengths with a length-1 item, both masks
    c.append(case("module-24-48-k3", 24, 48, 3, 17, B=3, in_lens=(17, 9, 1), out_lens=(17, 9, 1)))
    # ---- the encoders' real widths at short lengths (FFN, prenet, MelEncoder init / term projection, duration predictor, multi-speaker FFN)
    c.append(case("ffn-192-768-k3", 192, 768, 3, 40, in_lens=(40, 23)))
    c.append(case("ffn-768-192-k3", 768, 192, 3, 40, in_lens=(40, 23), out_lens=(40, 23)))
    c.append(case("prenet-192-192-k5", 192, 192, 5, 70, in_lens=(70, 33)))
    c.append(case("proj-192-80-k1", 192, 80, 1, 70, out_lens=(70, 33)))
    c.append(case("init-80-192-k1", 80, 192, 1, 70, in_lens=(70, 33), x_grad=False))
    c.append(case("dp-256-1-k1", 256, 1, 1, 70, in_lens=(70, 33), out_lens=(70, 33)))
    c.append(case("ffn-256-768-k3", 256, 768, 3, 33, in_lens=(33, 20)))
    # ---- time edges: a single position, one below / at / one above the position chunk, a dilated halo across the chunk edge
    c.append(case("time-L1", 20, 40, 3, 1, B=3))
    for L in (CHUNK - 1, CHUNK, CHUNK + 1):
        c.append(case("time-L%d" % L, 20, 40, 3, L, B=3, in_lens=(L, L - 2, 1), out_lens=(L, L - 2, 1)))
    c.append(case("dil3-k5", 20, 40, 5, 70, dil=3, B=3, in_lens=(70, 66, 5), out_lens=(70, 66, 5)))
    # ---- the reduction over positions: several slices, and a trailing slice past the last chunk (it must still write its zeros)
    c.append(case("slices-3", 16, 16, 3, 2 * CHUNK + 1, B=3, in_lens=(129, 100, 1)))
    c.append(case("slice-empty", 129, 129, 11, 5 * CHUNK, B=5, in_lens=(320, 319, 200, 64, 1), out_lens=(320, 319, 200, 64, 1)))
    # ---- every mask combination, ragged with a length-1 item
    for tag, im, om in (("none", False, False), ("in", True, False), ("out", False, True), ("both", True, True)):
        c.append(case("mask-" + tag, 20, 40, 3, 70, B=3, in_lens=(70, 33, 1) if im else None, out_lens=(70, 33, 1) if om else None))
    # ---- no bias gradient asked for; an input that needs no gradient
    c.append(case("no-bias", 20, 40, 3, 70, B=3, in_lens=(70, 33, 1), out_lens=(70, 33, 1), bias=False))
    c.append(case("no-dx", 20, 40, 3, 70, B=3, in_lens=(70, 33, 1), out_lens=(70, 33, 1), x_grad=False))
    return c


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
# what the weight-gradient launcher must choose for a named case: (slices, chunks per slice, empty slices)
EXPECT = {"module-24-48-k3": (1, 3, 0), "time-L63": (1, 3, 0), "time-L64": (1, 3, 0), "time-L65": (2, 3, 0), "slices-3": (3, 3, 0),
          "slice-empty": (6, 5, 1), "ffn-192-768-k3": (1, 2, 0)}


def _mask(lens, B, L):
    if lens is None:
        return None
    assert len(lens) == B and max(lens) <= L
    return seq_mask(lens, L)


def make_inputs(c):
    """CPU fp32 tensors of one case: x and dy standard normal, weights uniform at the 1 / sqrt(cin K) scale, 0 / 1 masks from the lengths."""
    g = torch.Generator().manual_seed(2000 + CASES.index(c))
    return dict(x=torch.randn(c.B, c.cin, c.L, generator=g), dy=torch.randn(c.B, c.cout, c.L, generator=g),
                w=(torch.rand(c.cout, c.cin, c.K, generator=g) * 2 - 1) / (c.cin * c.K) ** 0.5,
                bias=(torch.rand(c.cout, generator=g) - 0.5) if c.bias else None,
                in_mask=_mask(c.in_lens, c.B, c.L), out_mask=_mask(c.out_lens, c.B, c.L))


def reference(c, d, dtype=torch.float64):
    """torch autograd on the CPU in `dtype`: {y, dx, dw, db} (db None without a bias; dx computed whether or not the case asks for it)."""
    t = lambda v: None if v is None else v.to(dtype)
    x, w = t(d["x"]).requires_grad_(True), t(d["w"]).requires_grad_(True)
    b = None if d["bias"] is None else t(d["bias"]).requires_grad_(True)
    xin = x if d["in_mask"] is None else x * t(d["in_mask"]).unsqueeze(1)
    y = F.conv1d(xin, w, b, padding=(c.K - 1) // 2 * c.dil, dilation=c.dil)
    if d["out_mask"] is not None:
        y = y * t(d["out_mask"]).unsqueeze(1)
    grads = torch.autograd.grad(y, [x, w] + ([] if b is None else [b]), t(d["dy"]))
    return dict(y=y.detach(), dx=grads[0], dw=grads[1], db=None if b is None else grads[2])


def _shift(v, o):
    """v[..., q + o], zero where q + o leaves [0, L)."""
    L = v.shape[-1]
    out = torch.zeros_like(v)
    if o >= 0 and o < L:
        out[..., :L - o] = v[..., o:]
    elif o < 0 and -o < L:
        out[..., -o:] = v[..., :L + o]
    return out


def _shift_flat(v, o):
    """The same read without the sample's bounds: position q + o of a row runs on into whatever follows it in the [B][C][L] memory."""
    return _shift(v.reshape(-1), o).reshape(v.shape)


MISTAKES = ("taps_not_reversed", "offset_sign", "no_in_mask_on_x", "no_out_mask_on_dy", "halo_reads_neighbour", "last_chunk_dropped",
            "channels_not_swapped")


def formulas(c, d, mistake=None, dtype=torch.float64):
    """{dx, dw, db} from the formulas in the module docstring, in `dtype` on the CPU.  `mistake` restates one way a kernel could be wrong."""
    assert mistake is None or mistake in MISTAKES
    t = lambda v: None if v is None else v.to(dtype)
    x, w, dy = t(d["x"]), t(d["w"]), t(d["dy"])
    im = torch.ones(c.B, 1, c.L, dtype=dtype) if d["in_mask"] is None else t(d["in_mask"]).unsqueeze(1)
    om = torch.ones(c.B, 1, c.L, dtype=dtype) if d["out_mask"] is None else t(d["out_mask"]).unsqueeze(1)
    dym = dy if mistake == "no_out_mask_on_dy" else dy * om
    xm = x if mistake == "no_in_mask_on_x" else x * im
    # ---- data gradient: the forward convolution on dy with the transposed, tap-reversed weight
    if mistake == "channels_not_swapped":
        wt = w.reshape(c.cin, c.cout, c.K).flip(-1)               # the module's memory taken for [cin][cout][K] as it is
    elif mistake == "taps_not_reversed":
        wt = w.transpose(0, 1)
    else:
        wt = w.transpose(0, 1).flip(-1)
    dx = F.conv1d(dym, wt.contiguous(), None, padding=(c.K - 1) // 2 * c.dil, dilation=c.dil) * im
    # ---- weight gradient, tap by tap
    n = c.L // CHUNK * CHUNK if mistake == "last_chunk_dropped" else c.L
    shift = _shift_flat if mistake == "halo_reads_neighbour" else _shift
    dw = torch.zeros(c.cout, c.cin, c.K, dtype=dtype)
    for k in range(c.K):
        off = (k - (c.K - 1) // 2) * c.dil
        xs = shift(xm, -off if mistake == "offset_sign" else off)
        dw[:, :, k] = torch.einsum("boq,biq->oi", dym[..., :n], xs[..., :n])
    db = dym[..., :n].sum((0, 2)) if c.bias else None
    return dict(dx=dx, dw=dw, db=db)
