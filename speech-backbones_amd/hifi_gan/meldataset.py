"""Log-mel front end -- drop-in for the tensor part of Grad-TTS/hifi-gan/meldataset.py:13-74 (DiffVC carries an identical copy):
`mel_spectrogram` with the reference's signature and return value, `MAX_WAV_VALUE` and the dynamic-range helpers.

`mel_spectrogram(y, ...)` on a HIP tensor with center=False is ONE launch of the kernel in csrc/mel.hip (plan and packed tables are
cached per configuration and device).  When y requires grad (the HiFi-GAN mel loss on the generated waveform) the same launch sits in
an autograd Function whose backward is csrc/mel_train.hip: the values are the same bits, and y gets its gradient.  On a CPU tensor (DataLoader workers), or with center=True, the same seven steps run as torch ops
written here: reflect pad, frame, periodic Hann window, one-sided DFT, sqrt(re^2 + im^2 + 1e-9), mel projection, log(max(., 1e-5)).
The filterbank is librosa's default (slaney scale and normalisation), computed by the library in float64 -- librosa is not needed.

One extension, the keyword `y_lengths`: see mel_spectrogram.  wav file I/O and the dataset class are not part of this module.
"""
import numpy as np
import torch

MAX_WAV_VALUE = 32768.0


def _backend():
    import importlib.util
    import os
    import sys
    try:
        from .. import _lib
        return _lib
    except (ImportError, ValueError):
        name = "gradtts_mi355x_lib"
        if name not in sys.modules:
            path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "_lib.py")
            spec = importlib.util.spec_from_file_location(name, path)
            mod = importlib.util.module_from_spec(spec)
            sys.modules[name] = mod
            spec.loader.exec_module(mod)
        return sys.modules[name]


def dynamic_range_compression(x, C=1, clip_val=1e-5):
    return np.log(np.clip(x, a_min=clip_val, a_max=None) * C)


def dynamic_range_decompression(x, C=1):
    return np.exp(x) / C


def dynamic_range_compression_torch(x, C=1, clip_val=1e-5):
    return torch.log(torch.clamp(x, min=clip_val) * C)


def dynamic_range_decompression_torch(x, C=1):
    return torch.exp(x) / C


def spectral_normalize_torch(magnitudes):
    return dynamic_range_compression_torch(magnitudes)


def spectral_de_normalize_torch(magnitudes):
    return dynamic_range_decompression_torch(magnitudes)


_plans = {}         # configuration -> MelPlan
_blobs = {}         # (configuration, device) -> packed tables of the kernel
_basis = {}         # (configuration, device, dtype) -> (filterbank, window) of the torch path


def _plan(cfg):
    if cfg not in _plans:
        _plans[cfg] = _backend().MelPlan(*cfg)
    return _plans[cfg]


def _blob(cfg, device):
    key = (cfg, str(device))
    if key not in _blobs:
        _blobs[key] = _plan(cfg).pack(device)
    return _blobs[key]


class _KernelMel(torch.autograd.Function):
    """The kernel path under autograd: forward is the gtts_mel_forward launch (the values of the no-grad path bit for bit), backward
    the two launches of csrc/mel_train.hip, which form the frame spectra again from y -- nothing else is saved."""

    @staticmethod
    def forward(ctx, y, cfg, lens):
        ctx.cfg, ctx.lens = cfg, lens
        ctx.save_for_backward(y)
        return _plan(cfg).forward(_blob(cfg, y.device), y, lens)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dmel):
        y, = ctx.saved_tensors
        return _plan(ctx.cfg).backward(_blob(ctx.cfg, y.device), y, dmel, ctx.lens), None, None


def _kernel(y, cfg, lens=None):
    """The kernel on a HIP tensor; differentiable exactly when y requires grad in grad mode (float32 / contiguous conversion first, so a
    strided or float64 y gets its gradient through torch's own conversion)."""
    if torch.is_grad_enabled() and y.requires_grad:
        return _KernelMel.apply(y.to(torch.float32).contiguous(), cfg, lens)
    return _plan(cfg).forward(_blob(cfg, y.device), y, lens)


def _torch_recipe(y, cfg, center):
    """The seven steps in torch ops, on y's device and in y's floating dtype."""
    n_fft, _, _, hop, win, _, _ = cfg
    key = (cfg, str(y.device), y.dtype)
    if key not in _basis:
        _basis[key] = (_plan(cfg).filterbank().to(device=y.device, dtype=y.dtype),
                       torch.hann_window(win, dtype=y.dtype, device=y.device))
    fb, window = _basis[key]
    p = (n_fft - hop) // 2
    y = torch.nn.functional.pad(y.unsqueeze(1), (p, p), mode='reflect').squeeze(1)
    spec = torch.stft(y, n_fft, hop_length=hop, win_length=win, window=window, center=center, pad_mode='reflect', normalized=False,
                      onesided=True, return_complex=True)
    mag = torch.sqrt(spec.real.pow(2) + spec.imag.pow(2) + 1e-9)
    return spectral_normalize_torch(torch.matmul(fb, mag))


def mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False, y_lengths=None):
    """y [B, L] in [-1, 1] -> log-mel [B, num_mels, T] (meldataset.py:51-74).

    y_lengths (not in the reference): [B] ints (list, CPU or device tensor).  Row b is then the utterance y[b, :y_lengths[b]],
    reflected about its own ends; frames at or beyond its own count are 0, as both reference collate functions pad mels; the return
    value is (mel, mel_lengths) with mel_lengths an int64 tensor on y's device."""
    cfg = (int(n_fft), int(num_mels), int(sampling_rate), int(hop_size), int(win_size), float(fmin),
           float(sampling_rate) / 2 if fmax is None else float(fmax))
    if y.dim() != 2:
        raise RuntimeError("mel_spectrogram: y must be [B, L] (got %s)" % (tuple(y.shape),))
    if not y.is_floating_point():
        raise RuntimeError("mel_spectrogram: y must be a floating-point waveform in [-1, 1] (got %s); divide int16 samples by "
                           "MAX_WAV_VALUE first" % y.dtype)
    on_hip = y.is_cuda and not center
    if not y.is_cuda:       # (on a HIP tensor these two prints would cost a device synchronise per call: INTEGRATION.md)
        if torch.min(y) < -1.:
            print('min value is ', torch.min(y))
        if torch.max(y) > 1.:
            print('max value is ', torch.max(y))
    if y_lengths is None:
        return _kernel(y, cfg) if on_hip else _torch_recipe(y, cfg, center)

    p, B, L = (cfg[0] - cfg[3]) // 2, y.shape[0], y.shape[1]
    on_host = not (torch.is_tensor(y_lengths) and y_lengths.is_cuda)
    lens = torch.as_tensor(y_lengths).to(torch.int64).reshape(-1)
    if lens.numel() != B:
        raise RuntimeError("mel_spectrogram: y_lengths must hold one length per row of y")
    if on_host and (int(lens.min()) <= p or int(lens.max()) > L):
        raise RuntimeError("mel_spectrogram: every y_lengths entry must lie in (%d, %d]" % (p, L))
    span = 2 * p - (0 if center else cfg[0])          # center=True frames the row padded by n_fft / 2 more on both sides
    mel_lengths = torch.div(lens + span, cfg[3], rounding_mode='floor') + 1
    if on_hip:
        mel = _kernel(y, cfg, lens.to(device=y.device, dtype=torch.int32))
        return mel, mel_lengths.to(y.device)
    mel = y.new_zeros((B, cfg[1], (L + span) // cfg[3] + 1))
    for b, n in enumerate(lens.tolist()):
        row = _torch_recipe(y[b:b + 1, :n], cfg, center)
        mel[b, :, :row.shape[-1]] = row[0]
    return mel, mel_lengths.to(y.device)
