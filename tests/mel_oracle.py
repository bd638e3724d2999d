"""Test infrastructure of the log-mel front end (tests/test_mel_cpu.py, tests/test_gpu_mel.py): the seven steps of
mel_spectrogram(..., center=False) restated in torch on the CPU, the filterbank formula in float64, and the seeded test signals.
Nothing in the product imports this."""
import functools
import math

import torch

CFG1 = (1024, 80, 22050, 256, 1024, 0.0, 8000.0)        # n_fft, num_mels, sampling_rate, hop, win, fmin, fmax: both reference models
CFG2 = (512, 40, 16000, 160, 400, 50.0, 7600.0)         # win < n_fft, a hop that divides nothing, fmin > 0
SIGNALS = ("speechlike", "noise", "quiet", "zeros", "impulse")
ROWS = 3                                                # every signal is built with three rows; a test with B rows takes the first B


def hz_to_mel(f):
    return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def mel_to_hz(m):
    return m * (200.0 / 3.0) if m < 15.0 else 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0))


def mel_edges(cfg):
    """The num_mels + 2 band edges in Hz (float64)."""
    _, num_mels, _, _, _, fmin, fmax = cfg
    lo, hi = hz_to_mel(fmin), hz_to_mel(fmax)
    mels = torch.linspace(lo, hi, num_mels + 2, dtype=torch.float64)
    return torch.tensor([mel_to_hz(float(m)) for m in mels], dtype=torch.float64)


def filterbank64(cfg):
    """W [num_mels, n_fft / 2 + 1] in float64: slaney scale, slaney normalisation."""
    n_fft, num_mels, sr = cfg[0], cfg[1], cfg[2]
    f = mel_edges(cfg)
    fft = torch.linspace(0.0, sr / 2.0, n_fft // 2 + 1, dtype=torch.float64)
    lower = (fft[None, :] - f[:-2, None]) / (f[1:-1] - f[:-2])[:, None]
    upper = (f[2:, None] - fft[None, :]) / (f[2:] - f[1:-1])[:, None]
    return torch.clamp(torch.minimum(lower, upper), min=0.0) * (2.0 / (f[2:] - f[:-2]))[:, None]


def frames(cfg, L):
    return (L + 2 * ((cfg[0] - cfg[3]) // 2) - cfg[0]) // cfg[3] + 1


def recipe(y, cfg, dtype=torch.float64, center=False):
    """The seven steps on the CPU in `dtype`; the float64 filterbank is cast to float32 first, as the reference stores it."""
    n_fft, _, _, hop, win, _, _ = cfg
    p = (n_fft - hop) // 2
    y = torch.nn.functional.pad(y.to(dtype).unsqueeze(1), (p, p), mode="reflect")
    if center:                                          # torch.stft(center=True): n_fft / 2 more on both sides, reflected again
        y = torch.nn.functional.pad(y, (n_fft // 2, n_fft // 2), mode="reflect")
    fr = y.squeeze(1).unfold(-1, n_fft, hop)            # [B, T, n_fft]
    left = (n_fft - win) // 2
    window = torch.zeros(n_fft, dtype=dtype)
    window[left:left + win] = torch.hann_window(win, periodic=True, dtype=dtype)
    spec = torch.fft.rfft(fr * window, dim=-1)          # [B, T, n_fft / 2 + 1]
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9).transpose(1, 2)
    W = filterbank64(cfg).to(torch.float32).to(dtype)
    return torch.log(torch.clamp(torch.matmul(W, mag), min=1e-5))


@functools.lru_cache(maxsize=None)
def signal(name, L, sr=22050):
    """[ROWS, L] float32, |y| <= 1, built in float64 from a seed that depends on (name, L) only.  Callers must not modify it."""
    g = torch.Generator().manual_seed(1000 * SIGNALS.index(name) + L)
    t = torch.arange(L, dtype=torch.float64) / sr
    if name == "speechlike":
        rows = []
        for b in range(ROWS):
            f0 = 100.0 + 40.0 * b
            phase = 2 * math.pi * f0 * t - (0.01 * f0 / 3.0) * torch.cos(2 * math.pi * 3.0 * t)      # 3 Hz vibrato, 1 % deep
            v = sum(torch.sin(h * phase) / h for h in range(1, 40))
            v = v * (0.6 + 0.4 * torch.sin(2 * math.pi * 2.5 * t + b)) + 1e-3 * torch.randn(L, generator=g, dtype=torch.float64)
            rows.append(0.95 * v / v.abs().max())
        y = torch.stack(rows)
    elif name == "noise":
        y = (0.3 * torch.randn(ROWS, L, generator=g, dtype=torch.float64)).clamp(-1.0, 1.0)
    elif name == "quiet":
        y = 1e-4 * torch.randn(ROWS, L, generator=g, dtype=torch.float64)
    elif name == "zeros":
        y = torch.zeros(ROWS, L, dtype=torch.float64)
    else:                                               # impulse: a single 1.0 at sample 500 (rows shorter than that stay silent)
        y = torch.zeros(ROWS, L, dtype=torch.float64)
        if L > 500:
            y[:, 500] = 1.0
    return y.to(torch.float32)


@functools.lru_cache(maxsize=None)
def reference(name, cfg, L):
    """(float64 oracle [ROWS, num_mels, T], per-row max-abs error [ROWS] of the same recipe run in float32) on signal(name, L);
    computed once per process.  Callers must not modify it."""
    y = signal(name, L, cfg[2])
    ref = recipe(y, cfg)
    return ref, (recipe(y, cfg, torch.float32).double() - ref).abs().amax(dim=(1, 2))
