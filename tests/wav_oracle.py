"""Checker of the speaker encoder's waveform front end (csrc/wav.hip, diffvc/speaker_encoder/encoder/audio.py): the three steps restated
in torch on the CPU in a chosen dtype, and cached references on the seeded signals of mel_oracle / spk_oracle.

  kernel64(source_sr, sr)        torchaudio's default Resample kernel (sinc_interp_hann, width 6, rolloff 0.99), float64 [n, 2 w + o]
  resample(x, source_sr, dtype)  zero pad (w, w + o), strided conv1d with the kernel ROUNDED TO FP32 (what every implementation stores)
  normalize(x, ..., dtype)       normalize_volume_batch
  powmel(x, dtype)               reflect pad 200, frames of 400 at hop 160, periodic Hann, one-sided DFT, re^2 + im^2, slaney filterbank
                                 (float64 -> fp32, as stored), [B, T, 40]
  *_reference(...)               (float64 result, e_ref32 = max-abs error of the same recipe run in float32); cached: do not modify.
Nothing in the product imports this."""
import functools
import importlib
import math

import numpy as np
import torch

import mel_oracle as MO
import spk_oracle as SO

SR, N_FFT, HOP, N_MELS = 16000, 400, 160, 40
RATIOS = ((22050, 16000), (24000, 22050), (24000, 16000), (16000, 22050), (44100, 16000))
SPANS = {(22050, 16000): 17, (24000, 22050): 14, (24000, 16000): 19, (16000, 22050): 13, (44100, 16000): 34}


def audio():
    return importlib.import_module("speech-backbones_amd.diffvc.speaker_encoder.encoder.audio")


def reduced(source_sr, sr):
    g = math.gcd(source_sr, sr)
    return source_sr // g, sr // g


def resampled_length(L, source_sr, sr=SR):
    o, n = reduced(source_sr, sr)
    return -(-n * L // o)


@functools.lru_cache(maxsize=None)
def kernel64(source_sr, sr=SR, width=6, rolloff=0.99):
    """(k float64 [n, 2 w + o], unclamped t [n, 2 w + o], w, o, n)."""
    o, n = reduced(source_sr, sr)
    base = min(o, n) * rolloff
    w = int(math.ceil(width * o / base))
    p = torch.arange(n, dtype=torch.float64)[:, None]
    j = torch.arange(2 * w + o, dtype=torch.float64)[None, :]
    t_raw = (-p / n + (j - w) / o) * base
    t = t_raw.clamp(-width, width)
    sinc = torch.where(t == 0, torch.ones_like(t), torch.sin(math.pi * t) / (math.pi * torch.where(t == 0, torch.ones_like(t), t)))
    return (base / o) * torch.cos(t * math.pi / (2 * width)) ** 2 * sinc, t_raw, w, o, n


def resample(x, source_sr, dtype=torch.float64, sr=SR):
    k, _, w, o, n = kernel64(source_sr, sr)
    k = k.to(torch.float32).to(dtype)
    L = x.shape[-1]
    xp = torch.nn.functional.pad(x.to(dtype), (w, w + o))
    y = torch.nn.functional.conv1d(xp[:, None, :], k[:, None, :], stride=o)             # [B, n, L // o + 1]: y[b, p, q]
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :resampled_length(L, source_sr, sr)]


def normalize(x, target_dBFS, increase_only=False, decrease_only=False, dtype=torch.float64):
    x = x.to(dtype)
    change = target_dBFS - 10 * torch.log10(torch.mean(x ** 2, dim=-1))
    gain = 10 ** (change / 20)
    one = torch.ones_like(gain)
    gain = torch.where(change > 0, gain, one) if increase_only else torch.where(change < 0, gain, one) if decrease_only else one
    return x * gain[:, None]


def powmel(x, dtype=torch.float64):
    fb = torch.from_numpy(audio().mel_filterbank()).to(dtype)                            # float64 on the host, stored as fp32
    xp = torch.nn.functional.pad(x.to(dtype)[:, None, :], (N_FFT // 2, N_FFT // 2), mode="reflect")[:, 0]
    fr = xp.unfold(-1, N_FFT, HOP)                                                       # [B, T, 400]
    spec = torch.fft.rfft(fr * torch.hann_window(N_FFT, periodic=True, dtype=dtype), dim=-1)
    power = (spec.real ** 2 + spec.imag ** 2).transpose(1, 2)                            # [B, 201, T]
    return torch.transpose(torch.matmul(fb, power), 1, 2)


@functools.lru_cache(maxsize=None)
def wave(name, L, sr):
    """[3, L] float32: a mel_oracle signal, or 'harmonic' = three spk_oracle.harmonic_wav rows scaled to |y| < 1."""
    if name == "harmonic":
        y = np.stack([SO.harmonic_wav(L, 110.0 + 25.0 * b, seed=40 + b, sr=sr) for b in range(3)])
        return torch.from_numpy((0.9 * y / np.abs(y).max()).astype(np.float32))
    return MO.signal(name, L, sr)


@functools.lru_cache(maxsize=None)
def resample_reference(name, L, source_sr, sr=SR):
    x = wave(name, L, source_sr)
    ref = resample(x, source_sr, torch.float64, sr)
    return ref, float((resample(x, source_sr, torch.float32, sr).double() - ref).abs().max())


@functools.lru_cache(maxsize=None)
def powmel_reference(name, L):
    x = wave(name, L, SR)
    ref = powmel(x)
    return ref, float((powmel(x, torch.float32).double() - ref).abs().max())
