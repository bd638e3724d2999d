"""Inference entry points of the speaker encoder -- the functions of DiffVC/speaker_encoder/encoder/inference.py with the reference's
names, signatures and return types (DiffVC/inference.ipynb: `spk_encoder.load_model(path, device)`, `spk_encoder.embed_utterance(wav)`).

With the model on a HIP device embed_utterance and embed_utterance_batch hand the whole-utterance mel to the kernel once: the partial
utterances are addressed inside it (P = len(mel_slices), S = frame step, T = partial length) and the mean and renormalisation over them
come back from the same call.  On the CPU the same steps run in torch."""
from pathlib import Path

import numpy as np
import torch

from . import audio
from .audio import preprocess_wav, preprocess_wav_batch  # noqa: F401
from .model import SpeakerEncoder
from .params_data import *  # noqa: F401,F403
from .params_data import mel_window_step, partials_n_frames, sampling_rate

_model = None       # type: SpeakerEncoder
_device = None      # type: torch.device


def load_model(weights_fpath, device="cpu"):
    """Loads a reference checkpoint ({"model_state", "step"}) onto `device` (a torch device or its name; None: the GPU when there is
    one).  Outputs of the numpy entry points stay on the host."""
    global _model, _device
    if device is None:
        _device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    else:
        _device = torch.device(device)
    _model = SpeakerEncoder(_device, torch.device("cpu"))
    checkpoint = torch.load(weights_fpath, map_location="cpu")
    _model.load_state_dict(checkpoint["model_state"])
    _model.eval()
    print("Loaded encoder \"%s\" trained to step %d" % (Path(weights_fpath).name, checkpoint["step"]))


def is_loaded():
    return _model is not None


def _loaded():
    if _model is None:
        raise Exception("Model was not loaded. Call load_model() before inference.")
    return _model


def embed_frames_batch(frames, use_torch=False):
    """frames [batch, n_frames, n_channels] (numpy, or a tensor with use_torch) -> embeddings [batch, model_embedding_size]."""
    model = _loaded()
    if not use_torch:
        frames = torch.from_numpy(frames)
    with torch.no_grad():
        embeds = model.forward(frames.to(_device))
    return embeds if use_torch else embeds.detach().cpu().numpy()


def compute_partial_slices(n_samples, partial_utterance_n_frames=partials_n_frames, min_pad_coverage=0.75, overlap=0.5):
    """Where to cut a waveform of n_samples and its mel into partial utterances of partial_utterance_n_frames frames each, `overlap`
    of a partial shared with the next.  Returns (wav_slices, mel_slices); the last slice may reach beyond the waveform (pad it with
    zeros up to wav_slices[-1].stop) and is dropped when less than min_pad_coverage of it is covered, unless it is the only one."""
    assert 0 <= overlap < 1
    assert 0 < min_pad_coverage <= 1
    samples_per_frame = int(sampling_rate * mel_window_step / 1000)
    n_frames = int(np.ceil((n_samples + 1) / samples_per_frame))
    frame_step = max(int(np.round(partial_utterance_n_frames * (1 - overlap))), 1)
    starts = range(0, max(1, n_frames - partial_utterance_n_frames + frame_step + 1), frame_step)
    mel_slices = [slice(i, i + partial_utterance_n_frames) for i in starts]
    wav_slices = [slice(i * samples_per_frame, (i + partial_utterance_n_frames) * samples_per_frame) for i in starts]
    last = wav_slices[-1]
    if (n_samples - last.start) / (last.stop - last.start) < min_pad_coverage and len(mel_slices) > 1:
        mel_slices, wav_slices = mel_slices[:-1], wav_slices[:-1]
    return wav_slices, mel_slices


def _geometry(mel_slices):
    step = mel_slices[1].start - mel_slices[0].start if len(mel_slices) > 1 else 0
    return len(mel_slices), step, mel_slices[0].stop - mel_slices[0].start


def embed_utterance(wav, using_partials=True, return_partials=False, **kwargs):
    """wav: a preprocessed waveform (float numpy array) -> its embedding, float32 numpy [model_embedding_size], unit norm.
    using_partials=False feeds the whole mel as one sequence.  return_partials: (embed, partial embeddings [n_partials, E],
    wav slices), the last two None without partials.  kwargs go to compute_partial_slices."""
    model = _loaded()
    on_hip = _device.type == "cuda"
    if not using_partials:
        if on_hip:
            frames = audio.wav_to_mel_spectrogram_batch(torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)).to(_device)[None])
            embed = embed_frames_batch(frames, use_torch=True)[0].cpu().numpy()
        else:
            embed = embed_frames_batch(audio.wav_to_mel_spectrogram(wav)[None, ...])[0]
        return (embed, None, None) if return_partials else embed

    wave_slices, mel_slices = compute_partial_slices(len(wav), **kwargs)
    max_wave_length = wave_slices[-1].stop
    if max_wave_length >= len(wav):
        wav = np.pad(wav, (0, max_wave_length - len(wav)), "constant")
    if on_hip:
        wavs = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)).to(_device)[None]
        with torch.no_grad():
            partial, utt = model.forward_partials(audio.wav_to_mel_spectrogram_batch(wavs).contiguous(), *_geometry(mel_slices))
        embed, partial_embeds = utt[0].cpu().numpy(), (partial.cpu().numpy() if return_partials else None)
    else:
        frames = audio.wav_to_mel_spectrogram(wav)
        partial_embeds = embed_frames_batch(np.array([frames[s] for s in mel_slices]))
        raw_embed = np.mean(partial_embeds, axis=0)
        embed = raw_embed / np.linalg.norm(raw_embed, 2)
    return (embed, partial_embeds, wave_slices) if return_partials else embed


def embed_utterance_batch(wavs, using_partials=True, return_partials=False, **kwargs):
    """wavs [B, L] (tensor) -> embeddings [B, model_embedding_size] as a tensor on the model's device; with return_partials also the
    partial embeddings [B, n_partials, E] and the wav slices.  A batch too short for its last partial is padded with ONES, as the
    reference does (inference.py:171)."""
    model = _loaded()
    if not using_partials:
        embeds = embed_frames_batch(audio.wav_to_mel_spectrogram_batch(wavs.to(_device)).contiguous(), use_torch=True)
        return (embeds, None, None) if return_partials else embeds

    wave_slices, mel_slices = compute_partial_slices(wavs.shape[-1], **kwargs)
    max_wave_length = wave_slices[-1].stop
    if max_wave_length >= wavs.shape[-1]:
        wavs = torch.cat([wavs, torch.ones((wavs.shape[0], max_wave_length - wavs.shape[-1]), dtype=wavs.dtype, device=wavs.device)], 1)
    frames = audio.wav_to_mel_spectrogram_batch(wavs.to(_device)).contiguous()
    with torch.no_grad():
        partial, embeds = model.forward_partials(frames, *_geometry(mel_slices))
    if return_partials:
        return embeds, partial.view(wavs.shape[0], len(mel_slices), -1), wave_slices
    return embeds


def embed_speaker(wavs, **kwargs):
    raise NotImplementedError("embed_speaker is not implemented (nor is it in the reference)")
