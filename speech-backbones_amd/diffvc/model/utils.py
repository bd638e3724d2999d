"""Helpers with the names of DiffVC/model/utils.py:16-110: the loss and length helpers, and the Fast Griffin-Lim vocoder `FastGL` with
its two sub-modules (`from model.utils import FastGL, sequence_mask` of DiffVC/train_dec.py and train_enc.py).

`FastGL.forward` on a float32 HIP tensor runs the kernels of csrc/fgl.hip: one launch per iteration (plan cached per configuration, the
packed tables per configuration and device, re-packed when `pi.mel_basis_inverse` has been replaced).  On any other tensor the same recipe
runs as torch ops written here, in the tensor's dtype.  Deviations from the reference, both in how a constant is rounded: the mel
filterbank is the library's own (`MelPlan.filterbank()`: librosa's default slaney filterbank, fmax = 8000 as the reference hard-codes it,
computed in float64 and rounded to fp32) and its pseudo-inverse is taken with numpy.linalg.pinv in float64 and rounded to fp32, where the
reference inverts in whatever dtype librosa returned; and the `window` buffers hold the Hann window computed in float64 and rounded to
fp32 -- the values of the kernels' table -- where the reference evaluates it in fp32 (a last-place difference).  The kernel path takes
its window from that table, not from the buffers.  librosa and torchaudio are not needed.
"""
import weakref

import numpy as np
import torch

from ...model._backend import backend
from ...model.utils import convert_pad_shape, fix_len_compatibility, sequence_mask  # noqa: F401
from .base import BaseModule


def mse_loss(x, y, mask, n_feats):
    """utils.py:16-18."""
    return torch.sum(((x - y) ** 2) * mask) / (torch.sum(mask) * n_feats)


def _hann(n_fft):
    """The periodic Hann window as the kernels hold it: computed in float64, rounded to fp32."""
    return torch.hann_window(n_fft, periodic=True, dtype=torch.float64).float()


class PseudoInversion(BaseModule):
    """log-mel [B, n_mels, T] -> linear magnitudes [B, n_fft / 2 + 1, T] = pinv(mel filterbank) exp(log-mel) (utils.py:42-56).  The
    result can be negative; FastGL uses it as it is."""

    def __init__(self, n_mels, sampling_rate, n_fft):
        super(PseudoInversion, self).__init__()
        self.n_mels = n_mels
        self.sampling_rate = sampling_rate
        self.n_fft = n_fft
        mel_basis = backend().MelPlan(n_fft, n_mels, sampling_rate, n_fft // 4, n_fft, 0.0, 8000.0).filterbank()
        mel_basis_inverse = np.linalg.pinv(mel_basis.double().numpy())
        self.register_buffer("mel_basis_inverse", torch.from_numpy(mel_basis_inverse).float())

    def forward(self, log_mel_spectrogram):
        return torch.matmul(self.mel_basis_inverse.to(log_mel_spectrogram.dtype), torch.exp(log_mel_spectrogram))


class InitialReconstruction(BaseModule):
    """magnitudes [B, n_fft / 2 + 1, T] -> istft with zero phase [B, 1, hop_size (T - 1)] (utils.py:59-74)."""

    def __init__(self, n_fft, hop_size):
        super(InitialReconstruction, self).__init__()
        self.n_fft = n_fft
        self.hop_size = hop_size
        self.register_buffer("window", _hann(n_fft))

    def forward(self, stftm):
        spec = torch.complex(stftm, torch.zeros_like(stftm))
        x = torch.istft(spec, self.n_fft, hop_length=self.hop_size, win_length=self.n_fft, window=self.window.to(stftm.dtype), center=True)
        return x.unsqueeze(1)


_plans = {}         # (n_fft, n_mels, hop_size, momentum) -> FglPlan
_blobs = {}         # (configuration, device) -> (weak reference to the packed pi.mel_basis_inverse, its version, packed tables)


class FastGL(BaseModule):
    """Fast Griffin-Lim (utils.py:77-110): log-mel [B, n_mels, T] -> waveform [B, 1, hop_size (T - 1)]."""

    def __init__(self, n_mels, sampling_rate, n_fft, hop_size, momentum=0.99):
        super(FastGL, self).__init__()
        self.n_mels = n_mels
        self.sampling_rate = sampling_rate
        self.n_fft = n_fft
        self.hop_size = hop_size
        self.momentum = momentum
        self.pi = PseudoInversion(n_mels, sampling_rate, n_fft)
        self.ir = InitialReconstruction(n_fft, hop_size)
        self.register_buffer("window", _hann(n_fft))

    def _native(self, device):
        """The plan and the packed tables for `device`; packed again when pi.mel_basis_inverse is another tensor than the one packed
        (.to(), assignment) or has been written to since (load_state_dict copies in place and raises the version counter)."""
        cfg = (int(self.n_fft), int(self.n_mels), int(self.hop_size), float(self.momentum))
        if cfg not in _plans:
            _plans[cfg] = backend().FglPlan(*cfg)
        P = self.pi.mel_basis_inverse
        held = _blobs.get((cfg, str(device)))
        if held is None or held[0]() is not P or held[1] != P._version:
            held = (weakref.ref(P), P._version, _plans[cfg].pack(P, device))
            _blobs[(cfg, str(device))] = held
        return _plans[cfg], held[2]

    @torch.no_grad()
    def forward(self, s, n_iters=32):
        if s.dim() != 3 or s.shape[1] != self.n_mels:
            raise RuntimeError("FastGL: s must be [B, %d, T] (got %s)" % (self.n_mels, tuple(s.shape)))
        if self.hop_size * (s.shape[2] - 1) <= self.n_fft // 2:
            raise RuntimeError("FastGL: %d frames give %d samples, too few to reflect-pad by n_fft / 2 = %d; the smallest T is %d"
                               % (s.shape[2], self.hop_size * max(s.shape[2] - 1, 0), self.n_fft // 2,
                                  (self.n_fft // 2) // self.hop_size + 2))
        if s.is_cuda and s.dtype == torch.float32:
            plan, blob = self._native(s.device)
            return plan.forward(blob, s, n_iters).unsqueeze(1)
        return self._torch_recipe(s, n_iters)

    def _torch_recipe(self, s, n_iters):
        """The recipe in torch ops, on s's device and in s's dtype."""
        c = self.pi(s)
        x = self.ir(c).squeeze(1)
        window = self.window.to(s.dtype)
        prev_angles = torch.zeros_like(c)
        for _ in range(n_iters):
            spec = torch.stft(x, self.n_fft, hop_length=self.hop_size, win_length=self.n_fft, window=window, center=True,
                              pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
            angles = spec / torch.sqrt(torch.clamp(spec.real ** 2 + spec.imag ** 2, min=1e-8))
            spec = c * (angles + self.momentum * (angles - prev_angles))
            x = torch.istft(spec, self.n_fft, hop_length=self.hop_size, win_length=self.n_fft, window=window, center=True)
            prev_angles = angles
        return x.unsqueeze(1)
