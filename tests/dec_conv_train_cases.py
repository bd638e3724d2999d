"""Catalogue of single-op cases of the 2-D training convolutions of the decoder and of the DiffVC PostNet -- csrc/train.hip (forward and
data gradient on the inference kernels of conv_mfma.hip / conv_up.hip), train_wgrad.hip, train_wgrad7.hip, train_elem.hip and the
training ops of postnet.hip -- with their float64 reference, the formulas of the kernel headers restated in torch, a CPU emulation of
the documented split-bf16 arithmetic, and restated mistakes.  tests/test_gpu_dec_conv_train_ops.py runs every case on the GPU through the
wrappers of _lib.py; tests/test_dec_conv_train_cases_cpu.py proves without one that the bounds below tell the mistakes from the contract.

  op      wrappers (model/_train_ops.py Function)                                         tensors          arithmetic
  c3      conv3x3_masked / conv3x3_dgrad / conv3x3_wgrad, one or two sources (MaskedConv3x3)  y dx dw db       split-bf16
  c1      conv1x1_masked / conv1x1_dgrad / conv1x1_wgrad (MaskedConv1x1); variant `qkv` no mask, no bias; `out` bias only; `res` both
  c7      conv7x7_masked / conv7x7_dgrad / conv7x7_wgrad (MaskedConv7x7)                  y dx dw db       split-bf16
  dn      conv_resample(up=False); dx = add_masked(conv_resample(dy, dgrad_of_down=True)); dw, db = conv3x3_wgrad(x, zero_insert2(dy))
  up      conv_resample(up=True): y.  Its gradients exist only as the composition inside ResampleConv.backward and are held, with the
          same bounds, by the GPU test of the autograd Functions
  first   cin 2 or 3, k 3 or 1: y on the ragged-channel instance of conv_mfma.hip (split-bf16); dx conv_dgrad_small and dw, db
          gtts_conv_wgrad_small, whose headers (train_elem.hip) state plain fp32 fma sums -- fp32 ops
  final   final_conv_forward / final_conv_backward (FinalConv)                           y dx dw db       fp32
  pexp    postnet_expand; dx postnet_collapse, dw / db postnet_chan_dot (PostNetInitConv)                  fp32
  pcol    postnet_collapse; dx postnet_expand, dw postnet_chan_dot(want_sum=False), db postnet_chan_dot(v=None, mask=None,
          want_dot=False) (PostNetFinalConv)                                                                fp32
  zi s2d am amc   zero_insert2, space_to_depth2, add_masked (a given / None, mask given / None) and add_masked(channels=): `out` alone,
          which must equal the fp32 torch expression bit for bit (data movement and at most one fp32 add)

Value kinds, each on every convolution op (KINDS_OF):
  integers   x, dy, w, bias from {-3 .. 3}: exact in bf16, every partial sum below 2^24 (9 K < 2^24, K the longest contraction, asserted),
             so the result does not depend on split or order: the kernels must return the float64 reference EXACTLY.  The geometry test.
  plain      x, dy ~ N(0, 1), w uniform at the 1 / sqrt(cin k^2) scale
  offset30   x = 30 + N(0, 1)
  mishlike   x = Mish(2 N(0, 1)), dy = |N(0, 1)|: one-signed sums, what a Block convolution sees after GroupNorm + Mish
  range12    x and dy times 2^u per element, u uniform in {-12 .. 12}
The glue ops move data: `plain` and `integers` only (no arithmetic a value kind could stress).

Bounds.  ref = float64 autograd of the plain torch expression; M = the same expression on |x mask|, |w|, |dy|, |bias| (element for element).
  integers        got == ref in every element
  split-bf16      per element |got - ref| <= 2^-14 M (PER_ELEM): the scheme hi hi + lo hi + hi lo has an analytic worst case of 2^-15 M (two
                  operand residuals of 2^-17 and the dropped lo lo term of 2^-16), the same again is left for the fp32 accumulation;
                  per tensor e = max |got - ref| / max |ref| <= EMUL_FACTOR e_emul + 2e-6 and <= 1e-4, e_emul the same norm of
                  `emulate` (the documented arithmetic in fp32 torch on the CPU, per case)
  fp32            e <= 4 e_ref32 + 2e-6 and <= 1e-4, e_ref32 of fp32 autograd on the CPU; db of every op likewise (db_bound)
  zeros           dx is exactly 0 on every masked frame; every compared tensor has max |ref| > 0
Weight-gradient slices: tests/wgrad_regimes.regime proves (CPU test) the cases `slices-*` reach several slices, a trailing empty slice
and the unrolled loop of wgrad_reduce_kernel with a remainder, per kind.  Regimes that need more than about 1e6 elements per tensor
(every slice group unrolled: nslice >= 64 groups of 8) stay with tests/test_gpu_training_shapes.py.

Shapes are the smallest at which each geometry can go wrong; B = 2 with one full-length and one length-1 sample unless stated."""
import collections
import functools

import torch
import torch.nn.functional as F

from case_util import relerr, seq_mask  # noqa: F401

PER_ELEM = 2.0 ** -14
EMUL_FACTOR = 4.0
REL_CAP = 1e-4
ABS = 2e-6
KINDS = ("integers", "plain", "offset30", "mishlike", "range12")
CONV_OPS = ("c3", "c1", "c7", "dn", "up", "first", "final", "pexp", "pcol")
GLUE_OPS = ("zi", "s2d", "am", "amc")
KINDS_OF = dict({op: KINDS for op in CONV_OPS}, **{op: ("integers", "plain") for op in GLUE_OPS})
KSIZE = {"c3": 3, "c1": 1, "c7": 7, "dn": 3, "up": 4, "final": 1, "pexp": 1, "pcol": 1}

Case = collections.namedtuple("Case", "id op kind B cin cout H W lens c0 variant k")


def db_bound(e_ref32):
    """A plain fp32 sum: four times the error of the same sum in fp32 torch, plus 2e-6 for sums that fp32 torch gets exactly."""
    return min(4.0 * e_ref32 + ABS, REL_CAP)


def lengths(B, W):
    """Ragged utterance lengths as in tests/test_gpu_training_shapes.py: the first full, the second a single frame."""
    return tuple([W, 1][:B] + [1 + (37 * k + 11) % W for k in range(max(0, B - 2))])


def case(op, kind, cin, cout, H, W, B=2, lens=None, c0=0, variant="", k=None, tag=""):
    k = KSIZE.get(op, 1) if k is None else k
    cid = "%s%s-%s-b%d-%dto%d%s-%dx%d%s" % (op, ("-" + variant) if variant else "", kind, B, cin, cout, ("-c0.%d" % c0) if c0 else "", H, W,
                                        ("-" + tag) if tag else "")
    return Case(cid, op, kind, B, cin, cout, H, W, lengths(B, W) if lens is None else tuple(lens), c0, variant, k)


C3_CH = ((64, 64, 0), (128, 256, 0), (512, 128, 0), (256, 64, 128))
# 1x1, one pixel row / column, W below an 8-pixel block, W = 31 / 32 / 33 and 64 / 65, H = TR - 1, TR, TR + 1 for every tiling (full
# height TR = 8 at cout 64 and 4 above; half height 4 and 2): H in 1 2 3 4 5 7 8 9
C3_HW = ((1, 1), (1, 40), (5, 1), (3, 7), (9, 31), (9, 32), (9, 33), (8, 65), (7, 64), (4, 9), (2, 5))
C1_VAR = (("qkv", 64, 384), ("out", 128, 64), ("res", 256, 128))
C1_HW = ((1, 1), (9, 7), (2, 32), (5, 13), (3, 43))              # H W = 1, 63, 64, 65, 129; no row is a whole 64-pixel chunk
C7_CH = ((64, 64), (128, 128))
C7_HW = ((1, 1), (3, 3), (7, 63), (8, 64), (9, 65))
DN_HW = ((2, 2), (4, 34), (10, 66))
UP_HW = ((1, 1), (3, 17), (5, 33))
RS_CH = ((64, 64), (128, 128))
NONINT = KINDS[1:]


def _cases():
    c = []
    # ---- 3x3: every shape on every channel pair as `integers`; each other kind on each channel pair, walking through the shapes
    for ci, co, c0 in C3_CH:
        c += [case("c3", "integers", ci, co, H, W, c0=c0) for H, W in C3_HW]
    for n, (ci, co, c0) in enumerate(C3_CH):
        c += [case("c3", kind, ci, co, *C3_HW[3 + (n + 2 * j) % 8], c0=c0) for j, kind in enumerate(NONINT)]
    # a sample whose length is 0 mod 32 beside a length-1 one; a length-1 sample in the two-source layer is in every c0 case above
    c.append(case("c3", "integers", 64, 64, 3, 40, B=3, lens=(40, 32, 1), tag="len32"))
    c.append(case("c3", "plain", 256, 64, 3, 40, B=3, lens=(40, 32, 1), c0=128, tag="len32"))
    # the full-height instances: the smallest launches of 128 workgroups (the CPU test proves the instance)
    for kind in ("integers", "plain"):
        c.append(case("c3", kind, 64, 64, 121, 33, B=4, tag="full"))
        c.append(case("c3", kind, 128, 256, 61, 33, tag="full"))
    # ---- 1x1
    for var, ci, co in C1_VAR:
        c += [case("c1", "integers", ci, co, H, W, variant=var) for H, W in C1_HW]
        c += [case("c1", kind, ci, co, *C1_HW[1 + j], variant=var) for j, kind in enumerate(NONINT)]
    # ---- 7x7
    for ci, co in C7_CH:
        c += [case("c7", "integers", ci, co, H, W) for H, W in C7_HW]
        c += [case("c7", kind, ci, co, *C7_HW[1 + j]) for j, kind in enumerate(NONINT)]
    c.append(case("c7", "integers", 64, 64, 5, 9, lens=(1, 4), tag="len1-4"))
    c.append(case("c7", "plain", 64, 64, 5, 9, lens=(1, 4), tag="len1-4"))
    # ---- Downsample / Upsample and the pieces of ResampleConv.backward at their shapes
    for ci, co in RS_CH:
        c += [case("dn", "integers", ci, co, H, W) for H, W in DN_HW]
        c += [case("dn", kind, ci, co, *DN_HW[1 + j % 2]) for j, kind in enumerate(NONINT)]
        c += [case("up", "integers", ci, co, H, W) for H, W in UP_HW]
        c += [case("up", kind, ci, co, *UP_HW[1 + j % 2]) for j, kind in enumerate(NONINT)]
    for kind in KINDS_OF["zi"]:
        c += [case("zi", kind, 64, 64, H // 2, W // 2) for H, W in DN_HW]                  # dy of a Downsample
        c += [case("s2d", kind, 64, 64, 2 * H, 2 * W) for H, W in UP_HW]                    # dy of an Upsample
        for H, W in UP_HW + DN_HW[1:]:
            c += [case("am", kind, 64, 64, H, W, variant=v) for v in ("b*m", "a+b*m", "a+b")]
            c.append(case("amc", kind, 192, 64, H, W, c0=64))                               # channels [64, 128) of a 192-channel tensor
    # ---- first layer: cin 2 and 3, k 3 and 1, W = 1 / 7 / 45
    for ci in (2, 3):
        for k in (3, 1):
            c += [case("first", "integers", ci, 64, 5, W, k=k, tag="k%d" % k) for W in (1, 7, 45)]
    for j, kind in enumerate(NONINT):
        c.append(case("first", kind, 3, 64, 5, (7, 45)[j % 2], k=3, tag="k3"))
        c.append(case("first", kind, 2, 64, 5, (45, 7)[j % 2], k=1, tag="k1"))
    # ---- final_conv (64 -> 1, both masks) and the PostNet's single-channel convolutions
    for kind in KINDS:
        c += [case("final", kind, 64, 1, 80, 1), case("final", kind, 64, 1, 5, 45)]
    for op in ("pexp", "pcol"):
        ch = lambda C: (1, C) if op == "pexp" else (C, 1)
        for C in (64, 128):
            c += [case(op, "integers", *ch(C), H, W) for H, W in ((1, 1), (80, 7), (5, 129))]
        c += [case(op, kind, *ch((64, 128)[j % 2]), *((80, 7), (5, 129))[j % 2]) for j, kind in enumerate(NONINT)]
    # ---- the weight gradient's reduction over pixel slices (SLICES: what each case must reach, proved with wgrad_regimes.regime)
    c.append(case("c3", "plain", 64, 64, 9, 33, B=3, tag="slices"))
    c.append(case("c3", "integers", 512, 128, 10, 20, B=13, tag="slices-empty"))
    c.append(case("c3", "plain", 64, 64, 20, 416, tag="slices-rem"))
    c.append(case("c1", "plain", 128, 64, 9, 65, B=3, variant="out", tag="slices"))
    c.append(case("c1", "integers", 512, 512, 10, 65, B=3, variant="res", tag="slices-empty"))
    c.append(case("c1", "plain", 64, 64, 40, 416, B=1, lens=(300,), variant="res", tag="slices-rem"))
    c.append(case("c7", "plain", 64, 64, 9, 65, B=3, tag="slices"))
    c.append(case("c7", "integers", 128, 128, 13, 65, B=3, tag="slices-empty"))
    c.append(case("c7", "plain", 64, 64, 130, 70, B=1, lens=(61,), tag="slices-rem"))
    return c


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
# case tag -> the regime facts wgrad_regimes.regime must report (kind of the regime query from the op)
SLICES = {"slices": lambda r: r["nslice"] >= 3 and r["empty"] == 0, "slices-empty": lambda r: r["empty"] >= 1,
          "slices-rem": lambda r: r["remainder"]}
REGIME_KIND = {"c3": "3x3", "c1": "1x1", "c7": "7x7"}


def has_mask(c):
    return not (c.op == "c1" and c.variant in ("qkv", "out")) and not (c.op == "am" and c.variant == "a+b")


def has_bias(c):
    return not (c.op == "c1" and c.variant == "qkv")


def split_bf16(c, name):
    """Whether tensor `name` of the case comes from a split-bf16 kernel (else fp32)."""
    if c.op in ("c3", "c1", "c7", "dn", "up"):
        return name != "db"
    return c.op == "first" and name == "y"


def x_shape(c):
    return (c.B, c.H, c.W) if c.op == "pexp" else (c.B, c.cin, c.H, c.W)


def y_shape(c):
    if c.op == "dn":
        return (c.B, c.cout, c.H // 2, c.W // 2)
    if c.op == "up":
        return (c.B, c.cout, 2 * c.H, 2 * c.W)
    if c.op == "pcol":
        return (c.B, c.H, c.W)
    return (c.B, c.cout, c.H, c.W)


def w_shape(c):
    if c.op == "up":
        return (c.cin, c.cout, 4, 4)
    if c.op in ("pexp", "pcol"):
        return (max(c.cin, c.cout),)
    return (c.cout, c.cin, c.k, c.k)


def contraction(c):
    """The longest contraction of the case: input channels x taps (y), output channels x taps (dx), pixels (dw, db)."""
    return max(c.cin * c.k * c.k, c.cout * c.k * c.k, c.B * y_shape(c)[-1] * y_shape(c)[-2])


def _mask(c):
    return seq_mask(c.lens, c.W)


def _draw(kind, g, shape, role):
    """One tensor of a value kind; role "x" or "dy"."""
    if kind == "integers":
        return torch.randint(-3, 4, shape, generator=g).float()
    r = torch.randn(shape, generator=g)
    if kind == "offset30" and role == "x":
        return 30.0 + r
    if kind == "mishlike":
        return F.mish(2.0 * r) if role == "x" else r.abs()
    if kind == "range12":
        return r * torch.exp2(torch.randint(-12, 13, shape, generator=g).float())
    return r


# integer draws at 1 x 1 whose first seed leaves a gradient all zero (two draws of x both 0): the next seed (the CPU test holds max |ref| > 0)
RESEED = {"pexp-integers-b2-1to128-1x1": 1, "pcol-integers-b2-64to1-1x1": 1}


def make_inputs(c):
    """CPU fp32 tensors of one case: x, dy, w, bias (None without one), mask [B, W] (None without one); the glue ops: a, b, mask."""
    g = torch.Generator().manual_seed(9000 + CASES.index(c) + 1000 * RESEED.get(c.id, 0))
    if c.op in GLUE_OPS:
        b = _draw(c.kind, g, (c.B, c.cin, c.H, c.W), "x")
        a = _draw(c.kind, g, (c.B, c.cout, c.H, c.W), "dy") if c.op == "am" and c.variant != "b*m" else None
        return dict(a=a, b=b, mask=_mask(c) if has_mask(c) and c.op in ("am", "amc") else None)
    x, dy = _draw(c.kind, g, x_shape(c), "x"), _draw(c.kind, g, y_shape(c), "dy")
    nb = c.cout if c.op != "pcol" else 1
    if c.kind == "integers":
        w = torch.randint(-3, 4, w_shape(c), generator=g).float()
        bias = torch.randint(-3, 4, (nb,), generator=g).float()
    else:
        w = (torch.rand(w_shape(c), generator=g) * 2 - 1) / (c.cin * c.k * c.k) ** 0.5
        bias = torch.rand((nb,), generator=g) - 0.5
    return dict(x=x, dy=dy, w=w, bias=bias if has_bias(c) else None, mask=_mask(c) if has_mask(c) else None)


# ======================================================================================= the plain torch expression and its autograd
def _m4(mask, dtype):
    return 1.0 if mask is None else mask.to(dtype)[:, None, None, :]


def expression(c, x, w, b, mask):
    """The module's own expression of the op's forward on tensors of one dtype."""
    m = _m4(mask, x.dtype)
    if c.op in ("c3", "c7", "first", "c1"):
        return F.conv2d(x * m, w, b, padding=c.k // 2)
    if c.op == "dn":
        return F.conv2d(x * m, w, b, stride=2, padding=1)
    if c.op == "up":
        return F.conv_transpose2d(x * m, w, b, stride=2, padding=1)
    if c.op == "final":
        return F.conv2d(x * m, w, b) * m
    if c.op == "pexp":
        return F.conv2d((x * mask.to(x.dtype)[:, None, :]).unsqueeze(1), w.view(-1, 1, 1, 1), b)
    if c.op == "pcol":
        return F.conv2d(x * m, w.view(1, -1, 1, 1), b).squeeze(1)
    raise KeyError(c.op)


def reference(c, d, dtype=torch.float64, magnitude=False):
    """{y, dx, dw, db} (db None without a bias) by torch autograd on the CPU in `dtype`; magnitude: the same on |x|, |w|, |dy|, |bias| -- M."""
    t = (lambda v: None if v is None else v.abs().to(dtype)) if magnitude else (lambda v: None if v is None else v.clone().to(dtype))
    x, w = t(d["x"]).requires_grad_(True), t(d["w"]).requires_grad_(True)
    b = None if d["bias"] is None else t(d["bias"]).requires_grad_(True)
    y = expression(c, x, w, b, d["mask"])
    grads = torch.autograd.grad(y, [x, w] + ([] if b is None else [b]), t(d["dy"]))
    return dict(y=y.detach(), dx=grads[0], dw=grads[1], db=None if b is None else grads[2])


def glue_reference(c, d):
    """`out` of a glue op: the fp32 torch expression, which the kernels must equal bit for bit."""
    a, b, mask = d["a"], d["b"], d["mask"]
    if c.op == "zi":
        out = torch.zeros(c.B, c.cin, 2 * c.H, 2 * c.W)
        out[:, :, 0::2, 0::2] = b
        return out
    if c.op == "s2d":          # channel block (pr * 2 + pc): rows 2y + 1 - pr, columns 2x + 1 - pc
        return torch.cat([b[:, :, 1 - pr::2, 1 - pc::2] for pr in (0, 1) for pc in (0, 1)], 1)
    if c.op == "amc":
        b = b[:, c.c0:c.c0 + c.cout]
    bm = b if mask is None else b * mask[:, None, None, :]
    return bm if a is None else a + bm


# ==================================================================================== the kernel headers' formulas, restated in torch
MISTAKES = ("dgrad_taps_not_flipped", "channels_not_swapped", "wgrad_offset_sign", "wgrad_without_mask", "dgrad_without_omask",
            "edge_column_wraps", "row_halo_wraps", "last_column_chunk_dropped", "odd_last_row_dropped", "second_source_without_c0",
            "up_phase_parity_swapped", "down_padding_wrong_side", "down_fourth_tap_not_zero", "first_dgrad_without_mask",
            "final_without_output_mask", "collapse_bias_under_mask")
ARITHMETIC_MISTAKES = ("cross_term_dropped", "hi_by_truncation")
# the ops a geometry mistake is restated on
APPLIES = {"dgrad_taps_not_flipped": ("c3", "c7"), "channels_not_swapped": ("c3", "c1", "c7"), "wgrad_offset_sign": ("c3", "c7", "dn"),
           "wgrad_without_mask": ("c3", "c1", "c7", "dn", "first"), "dgrad_without_omask": ("c3", "c1", "c7", "dn"),
           "edge_column_wraps": ("c3", "c7", "first"), "row_halo_wraps": ("c3", "c7", "first"), "last_column_chunk_dropped": ("c3", "c1", "c7"),
           "odd_last_row_dropped": ("c3",), "second_source_without_c0": ("c3",), "up_phase_parity_swapped": ("up",),
           "down_padding_wrong_side": ("dn",), "down_fourth_tap_not_zero": ("dn",), "first_dgrad_without_mask": ("first",),
           "final_without_output_mask": ("final",), "collapse_bias_under_mask": ("pcol",)}


def applies(mistake, c):
    if c.op not in APPLIES[mistake]:
        return False
    if mistake == "second_source_without_c0":
        return c.c0 > 0
    if mistake in ("wgrad_without_mask", "dgrad_without_omask"):
        return has_mask(c)
    return True


def _shift(v, oy, ox):
    """v[..., y + oy, x + ox], zero where that leaves the plane."""
    H, W = v.shape[-2:]
    out = torch.zeros_like(v)
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 < y1 and x0 < x1:
        out[..., y0:y1, x0:x1] = v[..., y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def _flat(v, o):
    """v read o elements further on in its [B][C][H][W] memory, without any bounds but the tensor's own."""
    f = v.reshape(-1)
    out = torch.zeros_like(f)
    n = f.numel()
    if 0 <= o < n:
        out[:n - o] = f[o:]
    elif -n < o < 0:
        out[-o:] = f[:n + o]
    return out.reshape(v.shape)


def _shifter(mistake):
    """The tap read of a stride-1 convolution: (v, oy, ox) -> v[..., y + oy, x + ox]."""
    if mistake == "edge_column_wraps":            # the column offset applied to the flat index: an edge column reads the neighbouring row
        return lambda v, oy, ox: _flat(_shift(v, oy, 0), ox)
    if mistake == "row_halo_wraps":               # the row offset applied to the flat index: a halo row reads the neighbouring channel / sample
        return lambda v, oy, ox: _shift(_flat(v, oy * v.shape[-1]), 0, ox)
    return _shift


def _conv_taps(v, w, p, shift):
    """sum over taps of w[:, :, ky, kx] . v[..., y + ky - p, x + kx - p]  (w [cout][cin][k][k])."""
    k = w.shape[-1]
    return sum(torch.einsum("oi,bihw->bohw", w[:, :, ky, kx], shift(v, ky - p, kx - p)) for ky in range(k) for kx in range(k))


def _wgrad_taps(xm, dy, k, p, shift, sign=1):
    """dw[co][ci][ky][kx] = sum_{b,y,x} dy[b,co,y,x] xm[b,ci,y + ky - p,x + kx - p]."""
    dw = torch.zeros(dy.shape[1], xm.shape[1], k, k, dtype=xm.dtype)
    for ky in range(k):
        for kx in range(k):
            dw[:, :, ky, kx] = torch.einsum("bohw,bihw->oi", dy, shift(xm, sign * (ky - p), sign * (kx - p)))
    return dw


def _up_scatter(v, w4):
    """ConvTranspose2d 4x4 stride 2 pad 1: out[co][2 iy - 1 + ky][2 ix - 1 + kx] += w4[ci][co][ky][kx] v[ci][iy][ix]."""
    B, _, h, w = v.shape
    out = torch.zeros(B, w4.shape[1], 2 * h + 2, 2 * w + 2, dtype=v.dtype)
    for ky in range(4):
        for kx in range(4):
            out[:, :, ky:ky + 2 * h:2, kx:kx + 2 * w:2] += torch.einsum("io,bihw->bohw", w4[:, :, ky, kx], v)
    return out[:, :, 1:1 + 2 * h, 1:1 + 2 * w]


def _zero_insert(v):
    out = torch.zeros(v.shape[0], v.shape[1], 2 * v.shape[2], 2 * v.shape[3], dtype=v.dtype)
    out[:, :, 0::2, 0::2] = v
    return out


def formulas(c, d, mistake=None, dtype=torch.float64):
    """{y, dx, dw, db} from the formulas the kernel headers document (train.hip, train_wgrad.hip, train_wgrad7.hip, train_elem.hip,
    postnet.hip), in `dtype` on the CPU.  `mistake` restates one way a kernel could be wrong (a mistake that does not apply to the op
    changes nothing)."""
    assert mistake is None or mistake in MISTAKES
    if mistake is not None and not applies(mistake, c):
        mistake = None
    t = lambda v: None if v is None else v.to(dtype)
    x, w, dy, b = t(d["x"]), t(d["w"]), t(d["dy"]), t(d["bias"])
    mask = torch.ones(c.B, c.W, dtype=dtype) if d["mask"] is None else t(d["mask"])
    m = mask[:, None, None, :]
    shift = _shifter(mistake)
    db = None if b is None else dy.sum((0, 2, 3) if dy.dim() == 4 else (0, 1, 2)).reshape(b.shape)
    if c.op in ("c3", "c1", "c7", "first"):
        k, p = c.k, c.k // 2
        xm = x * m
        if mistake == "second_source_without_c0":      # channel ci >= c0 read at x1[ci] in place of x1[ci - c0]: c0 planes further on
            x1 = xm[:, c.c0:].contiguous()
            xm = torch.cat((xm[:, :c.c0], _flat(x1, c.c0 * c.H * c.W)), 1)
        bias4 = 0.0 if b is None else b.view(1, -1, 1, 1)
        y = _conv_taps(xm, w, p, shift) + bias4
        # data gradient: the forward convolution on dy with the weight transposed and its taps flipped, masked in the epilogue
        if mistake == "channels_not_swapped":
            wt = w.reshape(c.cin, c.cout, k, k).flip(-1, -2)
        elif mistake == "dgrad_taps_not_flipped":
            wt = w.transpose(0, 1)
        else:
            wt = w.transpose(0, 1).flip(-1, -2)
        dx = _conv_taps(dy, wt, p, shift)
        if mistake not in ("dgrad_without_omask", "first_dgrad_without_mask"):
            dx = dx * m
        # weight gradient, tap by tap, over the pixels of its chunks
        xw = x if mistake == "wgrad_without_mask" else xm
        dyw = dy
        if mistake == "last_column_chunk_dropped":
            n = {"c3": c.W // 32 * 32, "c7": c.W // 64 * 64}.get(c.op)
            if n is None:                              # 1x1: chunks of 64 pixels of the flattened plane
                keep = (torch.arange(c.H * c.W) < c.H * c.W // 64 * 64).to(dtype).view(1, 1, c.H, c.W)
                dyw = dy * keep
            else:
                dyw = dy * (torch.arange(c.W) < n).to(dtype).view(1, 1, 1, c.W)
        if mistake == "odd_last_row_dropped":
            dyw = dy * (torch.arange(c.H) < c.H // 2 * 2).to(dtype).view(1, 1, c.H, 1)
        dw = _wgrad_taps(xw, dyw, k, p, shift, -1 if mistake == "wgrad_offset_sign" else 1)
        if db is not None and dyw is not dy:
            db = dyw.sum((0, 2, 3))
        return dict(y=y, dx=dx, dw=dw, db=db)
    if c.op == "dn":
        # y[oy][ox] = sum w[ky][kx] xm[2 oy - 1 + ky][2 ox - 1 + kx]: the stride-1 sums at the even positions
        xm = x * m
        full = _conv_taps(xm, w, 0 if mistake == "down_padding_wrong_side" else 1, shift)
        y = full[:, :, 0::2, 0::2] + b.view(1, -1, 1, 1)
        # data gradient: an Upsample of dy with the forward weight zero-padded to 4x4 (ConvTranspose2d layout [in = cout][out = cin])
        w4 = F.pad(w, (0, 1, 0, 1))
        if mistake == "down_fourth_tap_not_zero":
            w4[:, :, 3, :], w4[:, :, :, 3] = w4[:, :, 2, :].clone(), w4[:, :, :, 2].clone()
        dx = _up_scatter(dy, w4)
        if mistake != "dgrad_without_omask":
            dx = dx * m
        # weight gradient: the stride-1 one against the zero-inserted dy
        dw = _wgrad_taps(x if mistake == "wgrad_without_mask" else xm, _zero_insert(dy), 3, 1, shift, -1 if mistake == "wgrad_offset_sign" else 1)
        return dict(y=y, dx=dx, dw=dw, db=db)
    if c.op == "up":
        xm = x * m
        y = _up_scatter(xm, w) + b.view(1, -1, 1, 1)
        if mistake == "up_phase_parity_swapped":       # even and odd output rows exchanged
            y = y.reshape(c.B, c.cout, c.H, 2, 2 * c.W).flip(3).reshape(y.shape)
        # dx[ci][iy][ix] = mask sum w[ci][co][ky][kx] dy[co][2 iy - 1 + ky][2 ix - 1 + kx]; dw the same products summed over pixels
        dyp = F.pad(dy, (1, 1, 1, 1))
        dx = torch.zeros_like(x)
        dw = torch.zeros_like(w)
        for ky in range(4):
            for kx in range(4):
                ph = dyp[:, :, ky:ky + 2 * c.H:2, kx:kx + 2 * c.W:2]
                dx += torch.einsum("io,bohw->bihw", w[:, :, ky, kx], ph)
                dw[:, :, ky, kx] = torch.einsum("bihw,bohw->io", xm, ph)
        return dict(y=y, dx=dx * m, dw=dw, db=db)
    if c.op == "final":
        # out = (sum_c w[c] x m + bias) m;  dx = w[c] dout m^2, dw[c] = sum dout m^2 x, db = sum dout m
        acc = torch.einsum("c,bchw->bhw", w.view(-1), x).unsqueeze(1) * m + b.view(1, 1, 1, 1)
        y = acc if mistake == "final_without_output_mask" else acc * m
        dm = dy if mistake == "final_without_output_mask" else dy * m
        return dict(y=y, dx=w.view(1, -1, 1, 1) * dm * m, dw=(dm * m * x).sum((0, 2, 3)).view(w.shape), db=dm.sum().view(1))
    if c.op == "pexp":
        # out[b,c,f,t] = w[c] x[b,f,t] mask[b,t] + bias[c]; dx = collapse(dy) (no bias), dw = chan_dot(dy, x, mask), db = sum dy
        xm = x * mask[:, None, :]
        y = w.view(1, -1, 1, 1) * xm.unsqueeze(1) + b.view(1, -1, 1, 1)
        return dict(y=y, dx=torch.einsum("c,bcft->bft", w, dy) * mask[:, None, :], dw=torch.einsum("bcft,bft->c", dy, xm), db=dy.sum((0, 2, 3)))
    if c.op == "pcol":
        # out[b,f,t] = sum_c w[c] x[b,c,f,t] mask[b,t] + bias; dx = expand(dy) (no bias), dw = chan_dot(x, dy, mask), db = sum dy
        acc = torch.einsum("c,bcft->bft", w, x) * mask[:, None, :]
        y = (acc + b) * mask[:, None, :] if mistake == "collapse_bias_under_mask" else acc + b
        dym = dy * mask[:, None, :]
        return dict(y=y, dx=w.view(1, -1, 1, 1) * dym.unsqueeze(1), dw=torch.einsum("bcft,bft->c", x, dym), db=dy.sum().view(1))
    raise KeyError(c.op)


# ============================================================================== the documented split-bf16 arithmetic, emulated in fp32
def _bf16(v, truncate=False):
    if truncate:
        return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return v.to(torch.bfloat16).float()


def _split(v, mistake):
    hi = _bf16(v, mistake == "hi_by_truncation")          # (lo stays round-to-nearest-even: |lo| doubles, and so does the dropped lo lo term)
    return hi, _bf16(v - hi)


def emulate(c, d, mistake=None):
    """The split-bf16 tensors of the case from hi hi + lo hi + hi lo with round-to-nearest-even bf16 parts and fp32 accumulation (fp32
    torch on the CPU; tests/numerics_emul.py scheme_bf16x3): y from (x mask, w), dx from (dy, w), dw from (dy, x mask).
    `mistake`: one of ARITHMETIC_MISTAKES."""
    assert mistake is None or mistake in ARITHMETIC_MISTAKES
    x, w, dy, b, mask = d["x"], d["w"], d["dy"], d["bias"], d["mask"]
    f = lambda xx, ww: expression(c, xx, ww, None, None)          # the bilinear map alone: no mask, no bias
    m = _m4(mask, torch.float32)
    xm = x * m

    def three(g, a, bb):
        (ah, al), (bh, bl) = _split(a, mistake), _split(bb, mistake)
        cross = g(al, bh) if mistake == "cross_term_dropped" else g(al, bh) + g(ah, bl)
        return g(ah, bh) + cross

    def dgrad(dyv, wv):
        x0 = torch.zeros_like(x).requires_grad_(True)
        return torch.autograd.grad(f(x0, wv), x0, dyv)[0]

    def wgrad(dyv, xv):
        w0 = torch.zeros_like(w).requires_grad_(True)
        return torch.autograd.grad(f(xv, w0), w0, dyv)[0]

    res = {}
    if split_bf16(c, "y"):
        res["y"] = three(f, xm, w) + (0.0 if b is None else b.view(1, -1, 1, 1))
    if split_bf16(c, "dx"):       # the 1x1 kernel masks dy on load (columns do not mix), the others the result in the epilogue
        res["dx"] = three(dgrad, dy * m, w) if c.op == "c1" else three(dgrad, dy, w) * m
    if split_bf16(c, "dw"):
        res["dw"] = three(wgrad, dy, xm)
    return res


# =========================================================================================================================== errors
def worst_ratio(got, ref, M):
    """max over elements of |got - ref| / M (an element with M = 0 must be exact: inf otherwise)."""
    err, M = (got.double() - ref.double()).abs(), M.double()
    r = torch.where(M > 0, err / M.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def instances(c, name_of):
    """{tensor: kernel instance} of the forward / data-gradient calls of a case that go through conv_train_launch.  name_of: the binding
    _lib.conv_train_kernel_name (the launching dispatch describing itself)."""
    if c.op in ("c3", "c1", "c7"):
        kind = {"c3": "3x3", "c1": "1x1", "c7": "7x7"}[c.op]
        return dict(y=name_of(kind, c.B, c.cin, c.cout, c.H, c.W, c0=c.c0), dx=name_of(kind, c.B, c.cout, c.cin, c.H, c.W))
    if c.op == "dn":
        return dict(y=name_of("dn", c.B, c.cin, c.cout, c.H, c.W), dx=name_of("up", c.B, c.cout, c.cin, c.H // 2, c.W // 2))
    if c.op == "up":
        return dict(y=name_of("up", c.B, c.cin, c.cout, c.H, c.W))
    if c.op == "first":
        return dict(y=name_of("3x3" if c.k == 3 else "1x1", c.B, c.cin, c.cout, c.H, c.W))
    return {}


def tensor_names(c):
    names = ["y"] if c.op == "up" else ["y", "dx", "dw"]
    return names + (["db"] if has_bias(c) and c.op != "up" else [])


def passes(c, name, got, ref, M, e_base):
    """The GPU bound of one tensor.  e_base: e_emul for a split-bf16 tensor, e_ref32 otherwise."""
    if c.kind == "integers":
        return bool(torch.equal(got.double(), ref.double()))
    e = relerr(got, ref)
    if split_bf16(c, name):
        return worst_ratio(got, ref, M) <= PER_ELEM and e <= min(EMUL_FACTOR * e_base + ABS, REL_CAP)
    return e <= db_bound(e_base)


@functools.lru_cache(maxsize=None)
def references(cid):
    """(case, inputs, ref64, M, e_base per tensor): computed once per process and never modified.  e_base is e_emul for the split-bf16
    tensors and e_ref32 for the others."""
    c = BY_ID[cid]
    d = make_inputs(c)
    ref, M, ref32, emu = reference(c, d), reference(c, d, magnitude=True), reference(c, d, torch.float32), emulate(c, d)
    base = {n: relerr(emu[n] if split_bf16(c, n) else ref32[n], ref[n]) for n in ("y", "dx", "dw", "db") if ref[n] is not None}
    return c, d, ref, M, base
