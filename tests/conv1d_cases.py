"""Catalogue of single-layer cases of the shared 1-D convolution kernel (csrc/conv1d.h) and their float64 reference.

tests/test_gpu_conv1d.py runs every case on the GPU through Conv1dOp; tests/test_conv1d_cases_cpu.py proves without a GPU that the
catalogue selects all nine kernel instances and every epilogue branch (Conv1dOp.instance: the launcher's own selection), that every
reference is finite and well above its bias, and that the bound tells a dropped cross-term MFMA, a shifted tap or a missing residual
from the kernel (CPU restatements of those mistakes).

Shapes are the smallest that still reach each mechanism: 16 input channels (one chunk) unless the case is about channels, B = 2 or 3 so
that a read across a sample boundary shows, lengths around the tile widths NT = 128 (128-row tile) and NT = 256 (64- / 32-row tiles)."""
import collections

import torch
import torch.nn.functional as F

from case_util import relerr, seq_mask  # noqa: F401

REL = 1e-4          # split-bf16 contractions, fp32 accumulate (tests/test_gpu_hifigan.py)

# epilogue ids of Conv1dOp.instance (csrc/conv1d.h, C1Epilogue)
EPI_BUFFER, EPI_UP16, EPI_UP8, EPI_GENERIC = 0, 1, 2, 3
EPI_NAME = {0: "buffer", 1: "up16", 2: "up8", 3: "generic"}
# (MT, TPS, AITER, KCH) of the nine compiled instances
INSTANCES = [(128, 3, 2, 1), (128, 4, 2, 1), (128, 3, 3, 1), (128, 4, 3, 1), (128, 3, 3, 2), (64, 3, 3, 1), (64, 4, 3, 1), (32, 3, 3, 1),
             (32, 4, 3, 1)]

Case = collections.namedtuple("Case", "id mode cin cout K dil S B Lin slope in_lens out_lens res accmode div")


def case(id, cin, cout, K, Lin, dil=1, S=1, B=2, slope=1.0, in_lens=None, out_lens=None, res=False, accmode=0, div=3.0):
    return Case(id, 0 if S == 1 else 1, cin, cout, K, dil, S, B, Lin, slope, in_lens, out_lens, res, accmode, div)


def _cases():
    c = []
    # ---- every instance (the 64- and 32-row ones again under "rows")
    c.append(case("inst-128-t3-a2", 16, 128, 3, 131))
    c.append(case("inst-128-t4-a2", 16, 128, 7, 131))
    c.append(case("inst-128-t3-a3-dil65", 16, 128, 3, 300, dil=65))          # halo 130: the first dilation past the AITER = 2 image
    c.append(case("inst-128-t3-a3-dil128", 32, 128, 3, 300, dil=128))        # halo 256: the launcher's limit on this tile
    c.append(case("inst-128-t4-a3-k5-dil40", 16, 128, 5, 300, dil=40))       # halo 160, two weight stages
    c.append(case("inst-128-t3-kch2", 64, 128, 3, 131))
    c.append(case("inst-64-t3", 16, 64, 3, 300))
    c.append(case("inst-64-t4", 16, 64, 5, 300))
    c.append(case("inst-32-t3", 16, 32, 3, 300))
    c.append(case("inst-32-t4", 16, 8, 7, 300))
    # ---- time edges per tile width, and inputs shorter than the halo
    for Lin in (1, 127, 128, 129, 259):
        c.append(case("time-nt128-L%d" % Lin, 16, 128, 3, Lin, B=3))
    for Lin in (1, 255, 256, 257, 515):
        c.append(case("time-nt256-L%d" % Lin, 16, 32, 3, Lin, B=3))
    for Lin in (3, 7):
        c.append(case("time-short-k11-dil5-L%d" % Lin, 16, 32, 11, Lin, dil=5, B=3))
    # ---- switches between instances
    c.append(case("switch-kch2-dil32", 32, 128, 3, 200, dil=32))
    c.append(case("switch-kch1-dil33", 32, 128, 3, 200, dil=33))
    c.append(case("switch-halo128-mt64", 16, 64, 3, 300, dil=64))
    c.append(case("switch-halo128-mt32", 16, 32, 3, 300, dil=64))
    for K in (1, 3, 5, 7, 11):                                               # one stage (padded taps), two stages, three stages
        c.append(case("taps-k%d" % K, 16, 64, K, 140))
    # ---- row edges: partial row tiles take the generic epilogue (bias clamp), whole ones the buffer epilogue
    for cout in (1, 4, 8, 31, 32, 33, 64, 96, 128, 160):
        c.append(case("rows-cout%d" % cout, 16, cout, 3, 70))
    # ---- input channels that do not fill a 16-channel chunk (pad channels must read as zero) and several chunks
    for cin, cout in ((4, 4), (8, 8), (20, 32), (40, 128), (48, 128)):
        c.append(case("cin%d-cout%d" % (cin, cout), cin, cout, 7, 70, B=3))
    # ---- ConvTranspose1d (kernel 2 S, padding S / 2)
    c.append(case("up-s2-two-stores", 16, 16, 4, 70, S=2, slope=0.1))        # M = 32, ls == 1: two 8-byte stores, adjacent channels
    c.append(case("up-s2-mt128", 32, 64, 4, 131, S=2, slope=0.1))
    c.append(case("up-s4-16byte", 16, 16, 8, 259, S=4, slope=0.1))           # M = 64, ls >= 2: one 16-byte store
    c.append(case("up-s8-16byte", 32, 16, 16, 131, S=8, slope=0.1))          # M = 128
    c.append(case("up-s2-partial-m8", 8, 4, 4, 70, S=2, slope=0.1))          # SMALL's last upsampler: generic epilogue
    c.append(case("up-s2-partial-m16", 16, 8, 4, 70, S=2, slope=0.1))
    c.append(case("up-s4-res-outmask", 16, 16, 8, 70, S=4, B=4, res=True, out_lens=(280, 121, 1, 0)))
    # ---- prologue and epilogue, on whole tiles (buffer epilogue) and partial ones (generic)
    for tag, cout in (("whole", 32), ("partial", 24)):
        for slope in (1.0, 0.1, 0.0):
            c.append(case("pro-%s-slope%g" % (tag, slope), 16, cout, 3, 70, slope=slope))
        c.append(case("pro-%s-masks" % tag, 16, cout, 5, 70, B=4, slope=0.0, in_lens=(70, 33, 1, 0), out_lens=(70, 33, 1, 0)))
        c.append(case("epi-%s-res" % tag, 16, cout, 3, 70, res=True))
        c.append(case("epi-%s-acc1" % tag, 16, cout, 3, 70, res=True, accmode=1))
        c.append(case("epi-%s-acc2" % tag, 16, cout, 3, 70, res=True, accmode=2, div=3.0))
        c.append(case("epi-%s-acc2-masks" % tag, 16, cout, 3, 70, B=4, slope=0.1, accmode=2, div=3.0, in_lens=(70, 33, 1, 0),
                      out_lens=(70, 33, 1, 0)))
    c.append(case("epi-mt128-res-acc2-masks", 16, 128, 3, 131, B=4, slope=0.1, res=True, accmode=2, in_lens=(131, 70, 1, 0),
                  out_lens=(131, 70, 1, 0)))
    return c


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
# what a named case must select: (MT, TPS, AITER, KCH), epilogue
EXPECT = {
    "inst-128-t3-a2": ((128, 3, 2, 1), EPI_BUFFER), "inst-128-t4-a2": ((128, 4, 2, 1), EPI_BUFFER),
    "inst-128-t3-a3-dil65": ((128, 3, 3, 1), EPI_BUFFER), "inst-128-t3-a3-dil128": ((128, 3, 3, 1), EPI_BUFFER),
    "inst-128-t4-a3-k5-dil40": ((128, 4, 3, 1), EPI_BUFFER), "inst-128-t3-kch2": ((128, 3, 3, 2), EPI_BUFFER),
    "inst-64-t3": ((64, 3, 3, 1), EPI_BUFFER), "inst-64-t4": ((64, 4, 3, 1), EPI_BUFFER), "inst-32-t3": ((32, 3, 3, 1), EPI_BUFFER),
    "inst-32-t4": ((32, 4, 3, 1), EPI_GENERIC),
    "switch-kch2-dil32": ((128, 3, 3, 2), EPI_BUFFER), "switch-kch1-dil33": ((128, 3, 2, 1), EPI_BUFFER),
    "switch-halo128-mt64": ((64, 3, 3, 1), EPI_BUFFER), "switch-halo128-mt32": ((32, 3, 3, 1), EPI_BUFFER),
    "rows-cout31": ((32, 3, 3, 1), EPI_GENERIC), "rows-cout33": ((32, 3, 3, 1), EPI_GENERIC), "rows-cout96": ((64, 3, 3, 1), EPI_GENERIC),
    "rows-cout160": ((128, 3, 2, 1), EPI_GENERIC), "cin48-cout128": ((128, 4, 2, 1), EPI_BUFFER),
    "up-s2-two-stores": ((32, 3, 3, 1), EPI_UP8), "up-s2-mt128": ((128, 3, 3, 2), EPI_UP8), "up-s4-16byte": ((64, 3, 3, 1), EPI_UP16),
    "up-s8-16byte": ((128, 3, 3, 2), EPI_UP16), "up-s2-partial-m8": ((32, 3, 3, 1), EPI_GENERIC),
    "up-s2-partial-m16": ((32, 3, 3, 1), EPI_GENERIC), "up-s4-res-outmask": ((64, 3, 3, 1), EPI_GENERIC),
    "epi-whole-acc2": ((32, 3, 3, 1), EPI_BUFFER), "epi-partial-acc2": ((32, 3, 3, 1), EPI_GENERIC),
}


def op_kwargs(c):
    return dict(mode=c.mode, cin=c.cin, cout=c.cout, K=c.K, dilation=c.dil, S=c.S)


def _mask(lens, B, L):
    if lens is None:
        return None
    assert len(lens) == B and max(lens) <= L
    return seq_mask(lens, L)


def make_inputs(c):
    """CPU fp32 tensors of one case: x standard normal (both signs), weights uniform at the 1 / sqrt(cin K) scale in the reference
    module's layout, the bias on the scale of the output, residual and running sum standard normal, 0 / 1 masks from the lengths."""
    g = torch.Generator().manual_seed(1000 + CASES.index(c))
    Lout = c.Lin * c.S
    wshape = (c.cout, c.cin, c.K) if c.mode == 0 else (c.cin, c.cout, c.K)
    # (a ConvTranspose1d output sees K / S = 2 of its K taps: its output, and with it the bias, is smaller by sqrt(2 / K))
    d = dict(x=torch.randn(c.B, c.cin, c.Lin, generator=g),
             w=(torch.rand(wshape, generator=g) * 2 - 1) / (c.cin * c.K) ** 0.5,
             bias=(torch.rand(c.cout, generator=g) - 0.5) * (1.0 if c.mode == 0 else (2.0 / c.K) ** 0.5),
             res=torch.randn(c.B, c.cout, Lout, generator=g) if c.res else None,
             accsrc=torch.randn(c.B, c.cout, Lout, generator=g) if c.accmode else None,
             in_mask=_mask(c.in_lens, c.B, c.Lin), out_mask=_mask(c.out_lens, c.B, Lout))
    assert bool((d["x"] > 0).any()) and bool((d["x"] < 0).any())
    return d


def reference(c, d, dtype=torch.float64, w=None, toff_shift=0, drop_res=False):
    """The layer in torch on the CPU in `dtype`, the epilogue in the kernel's order: + bias, + res, running sum, division, * out_mask.
    w / toff_shift / drop_res restate mistakes of the kernel for the sensitivity test (other weights, the LAST tap read one position
    late, no residual)."""
    t = lambda v: None if v is None else v.to(dtype)
    x, w = t(d["x"]), t(d["w"] if w is None else w)
    xin = F.leaky_relu(x, c.slope)
    if d["in_mask"] is not None:
        xin = xin * t(d["in_mask"]).unsqueeze(1)
    if c.mode == 0:
        pad = (c.K - 1) // 2 * c.dil
        y = F.conv1d(xin, w, None, padding=pad, dilation=c.dil)
        if toff_shift:        # take the last tap out of the true convolution and put it back reading toff_shift positions late
            off = (c.K - 1 - (c.K - 1) // 2) * c.dil

            def tap(o):       # sum_ci w[:, ci, K-1] x[ci, q + o], zero outside the input
                sh = torch.zeros_like(xin)
                if 0 <= o < c.Lin:
                    sh[..., :c.Lin - o] = xin[..., o:]
                return torch.einsum("oc,bcl->bol", w[:, :, -1], sh)
            y = y - tap(off) + tap(off + toff_shift)
    else:
        assert not toff_shift
        y = F.conv_transpose1d(xin, w, None, stride=c.S, padding=(c.K - c.S) // 2)
    v = y + t(d["bias"]).view(1, -1, 1)
    if d["res"] is not None and not drop_res:
        v = v + t(d["res"])
    if c.accmode == 1:
        v = t(d["accsrc"]) + v
    elif c.accmode == 2:
        v = (t(d["accsrc"]) + v) / c.div
    if d["out_mask"] is not None:
        v = v * t(d["out_mask"]).unsqueeze(1)
    return v


def bf16_round(w):
    return w.to(torch.bfloat16).to(torch.float32)
