"""Test infrastructure of the log-mel input gradient (tests/test_mel_grad_cases_cpu.py, tests/test_gpu_mel_grad.py): the catalogue of
cases, the float64 reference (autograd through mel_oracle.recipe), the same in float32 on the CPU (e_ref32), a hand-written float64
backward of the formulas the kernel implements (csrc/mel_train.hip) with the restated mistakes, and the error measure.
Nothing in the product imports this.

Error of a row: max-abs difference divided by the row's max |ref| (a row whose reference is all zero: 0 when the result is exactly
zero, inf otherwise).  GPU bound of a case: 4 e_ref32 + 2e-6 (the project's per-op bound) on every signal but speechlike, whose
gradient is ill-conditioned (quiet bins under a 1 / acc factor: e_ref32 itself reaches 2.6e-4 here and moves with the summation order);
there the bound is SPEECH_BOUND = 1e-2: about 40 times the worst float32 figure of this catalogue (2.6e-4) and a quarter of the
cheapest restated mistake on speechlike (a filter's last bin missing from the transposed table: 4e-2; the others cost 0.1 to 1).

Clip-side cells: a float32 kernel may land on the other side of the clip for cells within rounding of it.  dmel is zeroed on cells
whose float64 acc lies within relative 1e-3 of 1e-5 (never on `zeros`, where every cell is far below the clip)."""
import functools
import math

import torch

import mel_oracle as MO

L37 = 256 * 37 + 100
N256 = (256, 40, 16000, 64, 256, 0.0, 8000.0)
N2048F = (2048, 128, 44100, 512, 2048, 0.0, 22050.0)
N2048W = (2048, 80, 22050, 512, 1200, 0.0, 8000.0)
CFGS = {"cfg1": MO.CFG1, "cfg2": MO.CFG2, "n256": N256, "n2048-full": N2048F, "n2048-win1200": N2048W}
# amplitude of the half-clipped noise: 2e-5 and 3e-5 are given for cfg1 and cfg2 (10-14 % and ~47 % of cells on the clip, float64);
# the other three are chosen the same way, so that a part of the cells but not all of them sit on the clip (43 %, 7 %, 39 %)
HALFCLIP_AMP = {"cfg1": 2e-5, "cfg2": 3e-5, "n256": 8e-5, "n2048-full": 1.5e-5, "n2048-win1200": 6e-6}
SIGNALS = MO.SIGNALS + ("halfclip",)
SHAPES = [("cfg1", 385), ("cfg1", 845), ("cfg1", L37), ("cfg2", 160 * 59 + 31), ("n256", 64 * 41 + 9), ("n2048-full", 512 * 19 + 77),
          ("n2048-win1200", 512 * 19 + 77)]
RAGGED = ("cfg1", L37, (L37, 845, 385))
# (tag, L, lens or None, signal)
CASES = [(tag, L, None, name) for tag, L in SHAPES for name in SIGNALS] + [(RAGGED[0], RAGGED[1], RAGGED[2], name) for name in SIGNALS]
SPEECH_BOUND = 1e-2
CLIP, CLIP_BAND, CLIP_BAND_MAX_FRACTION = 1e-5, 1e-3, 0.01
MISTAKES = ("irfft", "halved", "imag_sign", "no_window", "no_clip_mask", "no_eps", "no_left_fold", "no_right_fold", "no_folds",
            "frame_origin", "ragged_frames_unmasked", "table_last_bin")


def case_id(case):
    tag, L, lens, name = case
    return "%s-L%d%s-%s" % (tag, L, "-ragged" if lens else "", name)


@functools.lru_cache(maxsize=None)
def signal(name, tag, L):
    """[ROWS, L] float32; callers must not modify it."""
    if name != "halfclip":
        return MO.signal(name, L, CFGS[tag][2])
    g = torch.Generator().manual_seed(7000 + L)
    return (HALFCLIP_AMP[tag] * torch.randn(MO.ROWS, L, generator=g, dtype=torch.float64)).to(torch.float32)


def window_of(cfg, dtype=torch.float64):
    n_fft, win = cfg[0], cfg[4]
    w = torch.zeros(n_fft, dtype=dtype)
    left = (n_fft - win) // 2
    w[left:left + win] = torch.hann_window(win, periodic=True, dtype=dtype)
    return w


def _acc(y, cfg, dtype):
    """W mag [B, num_mels, T] of the recipe, before clip and log."""
    n_fft, hop = cfg[0], cfg[3]
    p = (n_fft - hop) // 2
    yp = torch.nn.functional.pad(y.to(dtype).unsqueeze(1), (p, p), mode="reflect").squeeze(1)
    spec = torch.fft.rfft(yp.unfold(-1, n_fft, hop) * window_of(cfg, dtype), dim=-1)
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9).transpose(1, 2)
    return torch.matmul(MO.filterbank64(cfg).to(torch.float32).to(dtype), mag)


def autograd_grad(y, dmel, cfg, dtype):
    """d sum(mel dmel) / dy through mel_oracle.recipe in `dtype`, as float64."""
    y = y.to(dtype).clone().requires_grad_()
    (MO.recipe(y, cfg, dtype) * dmel.to(dtype)).sum().backward()
    return y.grad.double()


def rows_of(case):
    """[(row index, samples of the row)]"""
    _, L, lens, _ = case
    return [(b, (lens[b] if lens else L)) for b in range(MO.ROWS)]


@functools.lru_cache(maxsize=None)
def reference(case):
    """dict(y [ROWS, L] float32, dmel [ROWS, num_mels, T] float32 (clip-side cells zeroed), ref [ROWS, L] float64, e_ref32 [ROWS],
    band: fraction of the case's live cells zeroed, clipped: fraction of live cells on the clip).  Computed once per process; callers
    must not modify it."""
    tag, L, lens, name = case
    cfg = CFGS[tag]
    y = signal(name, tag, L)
    T = MO.frames(cfg, L)
    g = torch.Generator().manual_seed(31 * L + len(name) + (1 if lens else 0))
    dmel = torch.randn(MO.ROWS, cfg[1], T, generator=g, dtype=torch.float64).to(torch.float32)
    ref = torch.zeros(MO.ROWS, L, dtype=torch.float64)
    ref32 = torch.zeros(MO.ROWS, L, dtype=torch.float64)
    cells = banded = clipped = 0
    for b, n in rows_of(case):
        Tb = MO.frames(cfg, n)
        acc = _acc(y[b:b + 1, :n], cfg, torch.float64)[0]
        cells += acc.numel()
        clipped += int((acc < CLIP).sum())
        if name != "zeros":
            near = (acc - CLIP).abs() <= CLIP_BAND * CLIP
            banded += int(near.sum())
            dmel[b, :, :Tb][near] = 0.0
    for b, n in rows_of(case):
        Tb = MO.frames(cfg, n)
        ref[b, :n] = autograd_grad(y[b:b + 1, :n], dmel[b:b + 1, :, :Tb], cfg, torch.float64)[0]
        ref32[b, :n] = autograd_grad(y[b:b + 1, :n], dmel[b:b + 1, :, :Tb], cfg, torch.float32)[0]
    return dict(y=y, dmel=dmel, ref=ref, e_ref32=row_error(ref32, ref), band=banded / cells, clipped=clipped / cells)


def row_error(got, ref):
    """[rows] max-abs difference over the row's max |ref|; NaN counts as inf; an all-zero reference row: 0 if got is exactly 0, else inf."""
    got, ref = got.double(), ref.double()
    d = torch.nan_to_num((got - ref).abs(), nan=math.inf).amax(dim=1)
    scale = ref.abs().amax(dim=1)
    return torch.where(scale > 0, d / scale.clamp(min=1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, math.inf)))


def gpu_bound(case, e_ref32):
    """The bound tests/test_gpu_mel_grad.py asserts on a row with float32-reference error e_ref32."""
    return SPEECH_BOUND if case[3] == "speechlike" else 4.0 * float(e_ref32) + 2e-6


@functools.lru_cache(maxsize=None)
def _dft(n_fft):
    k = torch.arange(n_fft // 2 + 1, dtype=torch.float64)[:, None]
    n = torch.arange(n_fft, dtype=torch.float64)[None, :]
    ang = 2 * math.pi * ((k * n) % n_fft) / n_fft
    return torch.cos(ang), torch.sin(ang)


def _row_backward(yb, d, cfg, mistake=None):
    """yb [n] float64, d [num_mels, Tb] -> dy [n]: the formulas of csrc/mel_train.hip, one row."""
    n_fft, hop = cfg[0], cfg[3]
    p, n = (n_fft - hop) // 2, yb.numel()
    Tb = MO.frames(cfg, n)
    j = torch.arange(-p, n + p)
    j = j.abs()
    j = torch.where(j >= n, 2 * (n - 1) - j, j)
    win = window_of(cfg)
    X = torch.fft.rfft(yb[j].unfold(0, n_fft, hop)[:Tb] * win, dim=-1)                   # [Tb, K]
    mag = torch.sqrt(X.real ** 2 + X.imag ** 2 + (0.0 if mistake == "no_eps" else 1e-9))
    W = MO.filterbank64(cfg).to(torch.float32).double()                                # [num_mels, K]
    acc = W @ mag.t()                                                                  # [num_mels, Tb]
    dacc = d / acc if mistake == "no_clip_mask" else torch.where(acc >= CLIP, d / acc, torch.zeros_like(acc))
    Wt = W
    if mistake == "table_last_bin":                # the transposed table misses every filter's last bin
        Wt = W.clone()
        for i in range(W.shape[0]):
            nz = torch.nonzero(W[i]).flatten()
            if nz.numel():
                Wt[i, int(nz[-1])] = 0.0
    dmag = (Wt.t() @ dacc).t()                                                         # [Tb, K]
    G = dmag * (X.conj() if mistake == "imag_sign" else X) / mag
    if mistake == "irfft":                         # interior bins counted twice
        g = n_fft * torch.fft.irfft(G, n=n_fft, dim=-1)
    else:
        if mistake == "halved":                    # interior bins halved once more (with every filterbank here W[:, 0] = W[:, N/2] = 0, so
            G = G.clone()                          # halving DC and Nyquist as well would change nothing)
            G[:, 1:-1] *= 0.5
        C, S = _dft(n_fft)
        g = G.real @ C - G.imag @ S                                                    # Re sum_k G[k] e^{+2 pi i k n / N}
    dframe = g if mistake == "no_window" else g * win
    dpad = torch.zeros(n + 2 * p + (hop if mistake == "frame_origin" else 0), dtype=torch.float64)
    for t in range(Tb):
        o = (t + 1) * hop if mistake == "frame_origin" else t * hop
        dpad[o:o + n_fft] += dframe[t][:dpad.numel() - o]
    dpad = dpad[:n + 2 * p]
    dy = dpad[p:p + n].clone()
    if mistake not in ("no_left_fold", "no_folds"):
        dy[1:p + 1] += dpad[:p].flip(0)
    if mistake not in ("no_right_fold", "no_folds"):
        dy[n - 1 - p:n - 1] += dpad[p + n:].flip(0)
    return dy


def manual_grad(case, mistake=None):
    """The hand-written float64 backward on a case: [ROWS, L] float64."""
    tag, L, lens, _ = case
    cfg, r = CFGS[tag], reference(case)
    out = torch.zeros(MO.ROWS, L, dtype=torch.float64)
    for b, n in rows_of(case):
        Tb = MO.frames(cfg, n)
        yb = r["y"][b].double()
        out[b, :n] = _row_backward(yb[:n], r["dmel"][b, :, :Tb].double(), cfg, mistake)
        if mistake == "ragged_frames_unmasked" and Tb < r["dmel"].shape[-1]:
            d = r["dmel"][b].double().clone()
            d[:, :Tb] = 0.0                        # the frames behind the row's own count, formed from the whole padded row
            out[b] += _row_backward(yb, d, cfg)
    return out
