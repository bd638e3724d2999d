"""Test infrastructure of Fast Griffin-Lim (tests/test_fgl_cpu.py, tests/test_gpu_fgl.py): the recipe of DiffVC's FastGL written out
from its formulas in torch on the CPU, in a given dtype -- the pseudo-inverse projection, stft / istft with center = True as explicit
framing, real FFTs, overlap-add and envelope division -- plus the test mels and the spectral-convergence metric.  Nothing in the product
imports this.

A configuration is (n_fft, n_mels, sampling_rate, hop).  K = n_fft / 2 + 1, L = hop (T - 1)."""
import functools
import math

import numpy as np
import torch

import mel_oracle as MO

CFGA = (1024, 80, 22050, 256)
CFGB = (512, 40, 16000, 160)            # a hop that divides nothing: samples have 3 or 4 overlapping frames
MOMENTUM = 0.99
VARIANTS = ("momentum0", "stale_prev", "no_envelope", "trim_off_by_hop")     # the mistakes the metric must see


def mel_cfg(cfg):
    """The mel_oracle configuration whose filterbank FastGL inverts: win = n_fft, fmin = 0, fmax = 8000."""
    n_fft, n_mels, sr, hop = cfg
    return (n_fft, n_mels, sr, hop, n_fft, 0.0, 8000.0)


def min_frames(cfg):
    """The smallest T with hop (T - 1) > n_fft / 2."""
    return (cfg[0] // 2) // cfg[3] + 2


@functools.lru_cache(maxsize=None)
def basis64(cfg):
    """(W [n_mels, K] float64 holding the fp32-rounded filterbank, P [K, n_mels] float64 holding fp32(pinv64(W)), numpy's pinv as in
    the module, so that both start from the same matrix).  Do not modify."""
    W = MO.filterbank64(mel_cfg(cfg)).to(torch.float32).double()
    return W, torch.from_numpy(np.linalg.pinv(W.numpy())).to(torch.float32).double()


def window(cfg, dtype):
    return torch.hann_window(cfg[0], periodic=True, dtype=torch.float64).to(torch.float32).to(dtype)       # the fp32 buffer of the module


def stft(x, cfg, dtype=torch.float64):
    """x [B, L] -> complex [B, K, T]: reflect pad n_fft / 2, frames at stride hop, window, one-sided DFT."""
    n_fft, hop = cfg[0], cfg[3]
    y = torch.nn.functional.pad(x.to(dtype).unsqueeze(1), (n_fft // 2, n_fft // 2), mode="reflect").squeeze(1)
    fr = y.unfold(-1, n_fft, hop) * window(cfg, dtype)
    return torch.fft.rfft(fr, dim=-1).transpose(1, 2)


def istft(spec, cfg, envelope=True, trim=None):
    """complex [B, K, T] -> [B, L]: per-frame c2r (1 / n_fft, imaginary parts of DC and Nyquist ignored), times w, overlap-add in
    ascending frame order, divided by sum_t w^2, n_fft / 2 trimmed from both ends.  envelope / trim: the mutation switches."""
    n_fft, hop = cfg[0], cfg[3]
    B, _, T = spec.shape
    dtype = spec.real.dtype
    w = window(cfg, dtype)
    fr = torch.fft.irfft(spec.transpose(1, 2), n=n_fft, dim=-1) * w
    full = torch.zeros(B, n_fft + hop * (T - 1), dtype=dtype)
    env = torch.zeros(n_fft + hop * (T - 1), dtype=dtype)
    for t in range(T):
        full[:, t * hop:t * hop + n_fft] += fr[:, t]
        env[t * hop:t * hop + n_fft] += w * w
    lo = n_fft // 2 if trim is None else trim
    L = hop * (T - 1)
    if envelope:
        return full[:, lo:lo + L] / env[lo:lo + L]
    return full[:, lo:lo + L]


def project(logmel, cfg, dtype=torch.float64):
    """c [B, K, T] = P exp(logmel)."""
    return torch.matmul(basis64(cfg)[1].to(dtype), torch.exp(logmel.to(dtype)))


def init(logmel, cfg, dtype=torch.float64):
    """(c, x0)."""
    c = project(logmel, cfg, dtype)
    return c, istft(torch.complex(c, torch.zeros_like(c)), cfg)


def phases(s):
    return s / torch.sqrt(torch.clamp(s.real ** 2 + s.imag ** 2, min=1e-8))


def step(c, x, a_prev, cfg, dtype=torch.float64, momentum=MOMENTUM, variant=None):
    """One iteration in `dtype`: (x_out, a)."""
    c, a_prev = c.to(dtype), a_prev.to(torch.complex64 if dtype == torch.float32 else torch.complex128)
    a = phases(stft(x, cfg, dtype))
    m = 0.0 if variant == "momentum0" else momentum
    sp = c * (a + m * (a - a_prev))
    return istft(sp, cfg, envelope=variant != "no_envelope", trim=cfg[0] // 2 + cfg[3] if variant == "trim_off_by_hop" else None), a


def run(logmel, cfg, n_iters=32, dtype=torch.float64, momentum=MOMENTUM, variant=None):
    """The free-running recipe: x [B, L] after n_iters iterations."""
    c, x = init(logmel, cfg, dtype)
    a_prev = torch.zeros_like(torch.complex(c, c))
    for _ in range(n_iters):
        x, a = step(c, x, a_prev, cfg, dtype, momentum, variant)
        if variant != "stale_prev":
            a_prev = a
    return x


def spectral_convergence(x, c, cfg):
    """|| |stft64(x)| - c ||_F / || c ||_F, over the whole batch."""
    return float(torch.linalg.norm(stft(x.double(), cfg).abs() - c.double()) / torch.linalg.norm(c.double()))


@functools.lru_cache(maxsize=None)
def logmel(name, cfg, T):
    """[ROWS, n_mels, T] float32: the float64 recipe's log-mel of mel_oracle.signal(name), or all log(1e-5) for name 'floor'.  The signal
    has hop T samples, which mel_spectrogram(center = False) cuts into T frames.  Callers must not modify it."""
    if name == "floor":
        return torch.full((MO.ROWS, cfg[1], T), math.log(1e-5), dtype=torch.float32)
    L = cfg[3] * T
    m = MO.recipe(MO.signal(name, L, cfg[2]), mel_cfg(cfg))
    assert m.shape[-1] == T
    return m.to(torch.float32)
