"""Audio front end of the speaker encoder -- the functions of DiffVC/speaker_encoder/encoder/audio.py with torch and numpy alone.

The encoder's features are the POWER mel spectrogram (not log): n_fft = win = 400, hop 160, 40 slaney bands over 0 - 8000 Hz, centred
frames with reflect padding, periodic Hann window.  The batch functions -- preprocess_wav_batch, normalize_volume_batch,
wav_to_mel_spectrogram_batch -- run on the kernels of csrc/wav.hip when they are given a float32 HIP tensor that takes no part in
autograd (plan and packed tables cached per configuration and device), and as torch ops written here otherwise (CPU, float64, a
tensor that requires grad); the filterbank is computed here in float64 numpy, so librosa is not needed.
Optional packages: torchaudio is needed by nothing -- preprocess_wav_batch resamples with this module's own statement of
torchaudio's default Resample (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99).  librosa (file loading, resampling) and
webrtcvad (silence trimming) are imported by preprocess_wav alone, the numpy single-utterance path."""
import math
import struct
from pathlib import Path

import numpy as np
import torch

from .params_data import *  # noqa: F401,F403
from .params_data import (audio_norm_target_dBFS, mel_n_channels, mel_window_length, mel_window_step, sampling_rate,
                          vad_max_silence_length, vad_moving_average_width, vad_window_length)

int16_max = (2 ** 15) - 1


def _need(module, what):
    import importlib
    try:
        return importlib.import_module(module)
    except ImportError as e:
        raise RuntimeError("%s needs the `%s` package, which is not installed; pass a %d Hz waveform array and "
                           "trim_silence=False to run without it" % (what, module, sampling_rate)) from e


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f < 1000.0, f / (200.0 / 3.0), 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0))


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m < 15.0, m * (200.0 / 3.0), 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)))


def mel_filterbank(sr=sampling_rate, n_fft=None, n_mels=mel_n_channels, fmin=0.0, fmax=None):
    """librosa.filters.mel with its defaults (slaney scale, slaney area normalisation) as float32 [n_mels, n_fft // 2 + 1],
    computed in float64."""
    n_fft = int(sr * mel_window_length / 1000) if n_fft is None else int(n_fft)
    fmax = sr / 2.0 if fmax is None else float(fmax)
    bins = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    lower = (bins[None, :] - edges[:-2, None]) / (edges[1:-1] - edges[:-2])[:, None]
    upper = (edges[2:, None] - bins[None, :]) / (edges[2:] - edges[1:-1])[:, None]
    tri = np.maximum(0.0, np.minimum(lower, upper))
    return (tri * (2.0 / (edges[2:] - edges[:-2]))[:, None]).astype(np.float32)


_basis = {}         # (device, dtype) -> (filterbank, window)
_plans = {}         # source_sr -> WavPlan (host metadata: one per source rate serves every device)
_blobs = {}         # (source_sr, device) -> packed tables of the kernels
_kernels = {}       # (source_sr, target_sr, device, dtype) -> resampling kernel of the torch path


def _plan(source_sr=sampling_rate):
    if source_sr not in _plans:
        from .model import _backend
        _plans[source_sr] = _backend().WavPlan(source_sr, sampling_rate, int(sampling_rate * mel_window_length / 1000),
                                               int(sampling_rate * mel_window_step / 1000), mel_n_channels, 6, 0.99, 0.0, sampling_rate / 2.0)
    return _plans[source_sr]


def _blob(source_sr, device):
    key = (source_sr, str(device))
    if key not in _blobs:
        _blobs[key] = _plan(source_sr).pack(device)
    return _blobs[key]


def _on_kernels(wavs):
    """The kernels take float32 HIP tensors that autograd does not follow; everything else takes the torch ops."""
    return wavs.is_cuda and wavs.dtype == torch.float32 and wavs.dim() == 2 and not (torch.is_grad_enabled() and wavs.requires_grad)


def wav_to_mel_spectrogram_batch(wavs):
    """wavs [B, L] (torch, any device) -> power mel [B, 1 + L // hop, mel_n_channels]."""
    if _on_kernels(wavs):
        return _plan().powmel(_blob(sampling_rate, wavs.device), wavs)
    return _mel_torch(wavs)


def _mel_torch(wavs):
    """The power mel in torch ops, on wavs' device and in its dtype."""
    n_fft = int(sampling_rate * mel_window_length / 1000)
    hop = int(sampling_rate * mel_window_step / 1000)
    key = (str(wavs.device), wavs.dtype)
    if key not in _basis:
        _basis[key] = (torch.from_numpy(mel_filterbank()).to(wavs), torch.hann_window(n_fft).to(wavs))
    fb, window = _basis[key]
    s = torch.stft(wavs, n_fft=n_fft, hop_length=hop, win_length=n_fft, window=window, center=True, pad_mode="reflect",
                   return_complex=True)
    power = s.real ** 2 + s.imag ** 2
    return torch.transpose(torch.matmul(fb, power), 1, 2)


def wav_to_mel_spectrogram(wav):
    """wav: float numpy array [L] -> power mel as float32 numpy [1 + L // hop, mel_n_channels] (not log)."""
    wavs = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32))[None]
    return wav_to_mel_spectrogram_batch(wavs)[0].numpy().astype(np.float32)


def normalize_volume(wav, target_dBFS, increase_only=False, decrease_only=False):
    if increase_only and decrease_only:
        raise ValueError("Both increase only and decrease only are set")
    change = target_dBFS - 10 * np.log10(np.mean(wav ** 2))
    if (change < 0 and increase_only) or (change > 0 and decrease_only):
        return wav
    return wav * (10 ** (change / 20))


def normalize_volume_batch(wavs, target_dBFS, increase_only=False, decrease_only=False):
    if increase_only and decrease_only:
        raise ValueError("Both increase only and decrease only are set")
    if _on_kernels(wavs):
        return _plan().normalize(None, wavs, target_dBFS, increase_only, decrease_only)
    return _normalize_torch(wavs, target_dBFS, increase_only, decrease_only)


def _normalize_torch(wavs, target_dBFS, increase_only=False, decrease_only=False):
    """A row that is left alone is multiplied by exactly 1: an all-zero row is NaN (0 * inf) under increase_only and stays 0 otherwise
    (the reference's 1 + mask * (gain - 1) makes it NaN in every mode)."""
    change = target_dBFS - 10 * torch.log10(torch.mean(wavs ** 2, dim=-1))
    gain = 10 ** (change / 20)
    if increase_only:
        gain = torch.where(change > 0, gain, torch.ones_like(gain))
    elif decrease_only:
        gain = torch.where(change < 0, gain, torch.ones_like(gain))
    else:
        gain = torch.ones_like(gain)          # (as the reference: without a direction nothing is scaled)
    return wavs * gain.unsqueeze(-1)


def trim_long_silences(wav):
    """Keeps the voiced stretches of a waveform (webrtcvad, mode 3, on windows of vad_window_length ms; the flags are smoothed over
    vad_moving_average_width windows and widened by vad_max_silence_length windows on both sides)."""
    webrtcvad = _need("webrtcvad", "trim_long_silences")
    per_window = (vad_window_length * sampling_rate) // 1000
    wav = wav[:len(wav) - (len(wav) % per_window)]
    pcm = struct.pack("%dh" % len(wav), *(np.round(wav * int16_max)).astype(np.int16))
    vad = webrtcvad.Vad(mode=3)
    flags = np.array([vad.is_speech(pcm[2 * s:2 * (s + per_window)], sample_rate=sampling_rate)
                      for s in range(0, len(wav), per_window)], dtype=np.float64)
    width = vad_moving_average_width
    padded = np.concatenate((np.zeros((width - 1) // 2), flags, np.zeros(width // 2)))
    total = np.cumsum(padded)
    total[width:] = total[width:] - total[:-width]
    mask = np.round(total[width - 1:] / width).astype(bool)
    # binary dilation with a window of vad_max_silence_length + 1 flags
    r = vad_max_silence_length // 2
    wide = np.concatenate((np.zeros(r, dtype=bool), mask, np.zeros(vad_max_silence_length - r, dtype=bool)))
    mask = np.array([wide[i:i + vad_max_silence_length + 1].any() for i in range(len(mask))], dtype=bool)
    return wav[np.repeat(mask, per_window)]


def preprocess_wav(fpath_or_wav, source_sr=None, trim_silence=True):
    """A file path or a float waveform array -> the waveform the encoder was trained on: sampling_rate Hz, raised to
    audio_norm_target_dBFS when quieter, long silences removed.  trim_silence=False (not in the reference) skips the voice
    activity detection, so that an array at sampling_rate needs nothing beyond numpy."""
    if isinstance(fpath_or_wav, (str, Path)):
        wav, source_sr = _need("librosa", "loading an audio file").load(str(fpath_or_wav), sr=None)
    else:
        wav = fpath_or_wav
    if source_sr is not None and source_sr != sampling_rate:
        wav = _need("librosa", "resampling").resample(wav, orig_sr=source_sr, target_sr=sampling_rate)
    wav = normalize_volume(wav, audio_norm_target_dBFS, increase_only=True)
    if trim_silence:
        wav = trim_long_silences(wav)
    return wav


def resample_kernel(source_sr, target_sr=sampling_rate, lowpass_filter_width=6, rolloff=0.99):
    """The polyphase kernel of torchaudio.transforms.Resample with its defaults (sinc_interp_hann) -> (k float32 [n, 2 w + o] computed
    in float64, w, o, n) for the reduced rates o -> n: k[p][j] = (base / o) cos^2(t pi / (2 lpw)) sinc(t) with
    t = clamp((-p / n + (j - w) / o) base, -lpw, lpw), base = min(o, n) rolloff, w = ceil(lpw o / base)."""
    g = math.gcd(int(source_sr), int(target_sr))
    o, n = int(source_sr) // g, int(target_sr) // g
    base = min(o, n) * rolloff
    w = int(math.ceil(lowpass_filter_width * o / base))
    j = np.arange(-w, w + o, dtype=np.float64)[None, :] / o
    p = np.arange(0, -n, -1, dtype=np.float64)[:, None] / n
    t = np.clip((p + j) * base, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    sinc = np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t))
    return (sinc * window * (base / o)).astype(np.float32), w, o, n


def resample_batch(wavs, source_sr, target_sr=sampling_rate):
    """wavs [B, L] (two dimensions) at source_sr -> [B, ceil(n L / o)] at target_sr in torch ops, on wavs' device and in its dtype: one conv1d with
    stride o over the row zero-padded by w on the left and w + o on the right, the n phases interleaved."""
    if source_sr == target_sr:
        return wavs
    key = (int(source_sr), int(target_sr), str(wavs.device), wavs.dtype)
    if key not in _kernels:
        k, w, o, n = resample_kernel(source_sr, target_sr)
        _kernels[key] = (torch.from_numpy(k).to(wavs)[:, None, :], w, o, n)
    k, w, o, n = _kernels[key]
    L = wavs.shape[-1]
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(wavs, (w, w + o))[:, None, :], k, stride=o)      # [B, n, L // o + 1]
    return y.transpose(1, 2).reshape(wavs.shape[0], -1)[:, :-(-n * L // o)]


def _ratio_on_kernels(source_sr):
    """csrc/wav.hip holds one tap table per phase: it takes rates that reduce to o / n with both <= 1024 (gtts_wav_create)."""
    g = math.gcd(int(source_sr), sampling_rate)
    return source_sr == int(source_sr) and max(int(source_sr), sampling_rate) // g <= 1024


def preprocess_wav_batch(wavs, source_sr=22050):
    """wavs [B, L] at source_sr -> [B, ceil(n L / o)] at sampling_rate, raised to audio_norm_target_dBFS where quieter.  On the kernels:
    resample, then normalise with the tile sums the resampler left.  A source rate the kernels do not take (16010 Hz reduces to 1601 / 1600) is
    resampled by the torch recipe on the tensor's device."""
    if sampling_rate != source_sr and _on_kernels(wavs) and _ratio_on_kernels(source_sr):
        plan = _plan(int(source_sr))
        wavs, partials = plan.resample(_blob(int(source_sr), wavs.device), wavs)
        return plan.normalize(None, wavs, audio_norm_target_dBFS, increase_only=True, partials=partials)
    return normalize_volume_batch(resample_batch(wavs, source_sr), audio_norm_target_dBFS, increase_only=True)
