"""CPU: the speaker encoder's host side -- exported symbols, argument checks that touch no device, the drop-in package
diffvc/speaker_encoder/encoder (state_dict layout, partial slices against the reference's recorded output, the numpy filterbank against
the library's, the torch path of embed_utterance / embed_utterance_batch against the float64 recipe of tests/spk_oracle.py)."""
import ctypes
import importlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import spk_oracle as SO
import abi_util
from conftest import GOLDEN, ROOT, pkg


@pytest.fixture(scope="module")
def I(tmp_path_factory):
    mod = SO.encoder_pkg()
    sd = SO.state("default")
    sd.update(similarity_weight=torch.tensor([10.]), similarity_bias=torch.tensor([-5.]))
    path = tmp_path_factory.mktemp("spk") / "encoder.pt"
    torch.save({"model_state": sd, "step": 3}, path)
    mod.load_model(path, device="cpu")
    return mod


def test_spk_symbols_are_exported_and_the_abi_version_stays():
    S = pkg()
    exported = {n for n in abi_util.exported(S._lib.LIB_PATH) if n.startswith("gtts_spk_")}
    assert exported == {"gtts_spk_create", "gtts_spk_destroy", "gtts_spk_num_params", "gtts_spk_param_info", "gtts_spk_packed_bytes",
                        "gtts_spk_pack", "gtts_spk_workspace_bytes", "gtts_spk_forward"}
    header = open(os.path.join(ROOT, "include", "gradtts_abi.h")).read()
    assert exported == set(re.findall(r"\b(gtts_spk_[a-z_0-9]+)\s*\(", header))
    assert S._lib.lib().gtts_abi_version() == 7


def test_plan_layout_and_refusals_touch_no_device():
    S = pkg()
    L = S._lib.lib()
    plan = S.SpkPlan()
    sd = SO.state("default")
    assert plan.param_layout() == [(k, tuple(v.shape)) for k, v in sd.items()]
    assert plan.packed_bytes() >= sum(v.numel() * 4 for v in sd.values())
    assert plan.workspace_bytes(12, 160) >= 12 * 160 * (1024 + 256) * 4 and plan.workspace_bytes(17, 160) > plan.workspace_bytes(16, 160)
    for kw in (dict(hidden=128), dict(n_mels=41), dict(layers=0), dict(layers=9), dict(embed=0)):
        with pytest.raises(RuntimeError, match=r"\(-3\)"):               # GTTS_E_CONFIG
            S.SpkPlan(**kw)
    assert S.SpkPlan(n_mels=80, layers=2, embed=192).param_layout()[-2] == ("linear.weight", (192, 256))
    # slice geometry and sizes: GTTS_E_SHAPE before any pointer is followed (the pointers here are not addresses of anything)
    fake = ctypes.c_void_p(4096)
    fwd = lambda U, Tt, P, S_, T: L.gtts_spk_forward(plan._h, fake, fake, U, Tt, P, S_, T, fake, None, None, fake, 1 << 40, None)
    assert fwd(2, 400, 4, 80, 161) == -2 and b"beyond" in L.gtts_last_error()
    assert fwd(1, 160, 1, 0, 161) == -2 and fwd(1, 160, 2, 1, 160) == -2
    assert fwd(0, 160, 1, 0, 160) == -2 and fwd(1, 160, 0, 0, 160) == -2 and fwd(1, 160, 1, 0, 0) == -2 and fwd(1, 160, 1, -1, 160) == -2
    assert fwd(1 << 14, 160, 1, 0, 160) == -2 and plan.workspace_bytes(1 << 14, 160) == 0      # 2^14 * 160 * 1024 >= 2^31
    assert L.gtts_spk_forward(plan._h, fake, fake, 1, 160, 1, 0, 160, fake, None, None, fake, 1024, None) == -6     # workspace too small
    assert L.gtts_spk_forward(plan._h, fake, None, 1, 160, 1, 0, 160, fake, None, None, fake, 1 << 40, None) == -1
    # a wrong parameter list: GTTS_E_PARAMS
    arr = (ctypes.c_void_p * 13)(*([4096] * 13))
    assert L.gtts_spk_pack(plan._h, arr, 13, fake, None) == -5 and b"expected 14" in L.gtts_last_error()
    with pytest.raises(RuntimeError, match="missing 'linear.bias'"):
        plan.pack({k: v for k, v in sd.items() if k != "linear.bias"}, "cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        plan.forward(None, torch.zeros(1, 160, 40))


def test_compute_partial_slices_equals_the_reference(I):
    cases = json.load(open(os.path.join(GOLDEN, "spk_partial_slices.json")))["cases"]
    assert {c["n_samples"] for c in cases} == {1, 159, 25600, 25601, 38399, 38400, 160000, 16000 * 37 + 11}
    assert any("overlap" in c["kwargs"] for c in cases) and any("min_pad_coverage" in c["kwargs"] for c in cases)
    for c in cases:
        wav, mel = I.compute_partial_slices(c["n_samples"], **c["kwargs"])
        assert all(isinstance(s, slice) for s in wav + mel)
        assert [[int(s.start), int(s.stop)] for s in wav] == c["wav"], c["n_samples"]
        assert [[int(s.start), int(s.stop)] for s in mel] == c["mel"], c["n_samples"]
        # what the kernel path relies on: equal steps, equal lengths
        P, S_, T = I._geometry(mel)
        assert [[p * S_, p * S_ + T] for p in range(P)] == c["mel"]


def test_state_dict_and_constants(I):
    m = I.SpeakerEncoder("cpu", "cpu")
    want = [("similarity_weight", (1,)), ("similarity_bias", (1,))]
    for l in range(3):
        want += [("lstm.weight_ih_l%d" % l, (1024, 40 if l == 0 else 256)), ("lstm.weight_hh_l%d" % l, (1024, 256)),
                 ("lstm.bias_ih_l%d" % l, (1024,)), ("lstm.bias_hh_l%d" % l, (1024,))]
    want += [("linear.weight", (256, 256)), ("linear.bias", (256,))]
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    assert m.similarity_weight.item() == 10.0 and m.similarity_bias.item() == -5.0
    assert sum(p.numel() for p in m.parameters()) == 1423618
    P = importlib.import_module("speech-backbones_amd.diffvc.speaker_encoder.encoder.params_data")
    Q = importlib.import_module("speech-backbones_amd.diffvc.speaker_encoder.encoder.params_model")
    assert (P.mel_window_length, P.mel_window_step, P.mel_n_channels, P.sampling_rate, P.partials_n_frames, P.inference_n_frames,
            P.vad_window_length, P.vad_moving_average_width, P.vad_max_silence_length, P.audio_norm_target_dBFS) == \
        (25, 10, 40, 16000, 160, 80, 30, 8, 6, -30)
    assert (Q.model_hidden_size, Q.model_embedding_size, Q.model_num_layers, Q.learning_rate_init, Q.speakers_per_batch,
            Q.utterances_per_speaker) == (256, 256, 3, 1e-4, 64, 10)
    for name, args in (("similarity_matrix", (torch.zeros(2, 2, 256),)), ("loss", (torch.zeros(2, 2, 256),)), ("do_gradient_ops", ())):
        with pytest.raises(NotImplementedError, match="GE2E training"):
            getattr(m, name)(*args)


def test_numpy_filterbank_equals_the_library(I):
    S = pkg()
    fb = I.audio.mel_filterbank(16000, 512, 40, 0.0, 8000.0)
    lib = S.MelPlan(512, 40, 16000, 128, 512, 0.0, 8000.0).filterbank().numpy()
    assert fb.shape == lib.shape == (40, 257) and fb.dtype == np.float32
    assert float(np.abs(fb - lib).max()) <= 1e-6
    real = I.audio.mel_filterbank()
    assert real.shape == (40, 201) and bool((real.sum(1) > 0).all()) and float(real.min()) == 0.0


def test_power_mel_front_end(I):
    wav = SO.harmonic_wav(16000 + 37, 150.0, seed=1)
    mel = I.audio.wav_to_mel_spectrogram(wav)
    assert mel.shape == (1 + len(wav) // 160, 40) and mel.dtype == np.float32 and float(mel.min()) >= 0
    # float64 restatement: reflect pad n_fft / 2, frames of 400 at hop 160, periodic Hann, |DFT|^2, filterbank
    y = np.pad(wav.astype(np.float64), 200, mode="reflect")
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 400)
    fr = np.stack([y[160 * t:160 * t + 400] * win for t in range(mel.shape[0])])
    want = (np.abs(np.fft.rfft(fr, axis=1)) ** 2) @ I.audio.mel_filterbank().astype(np.float64).T
    assert float(np.abs(mel - want).max()) <= 1e-5 * float(want.max())
    batch = I.audio.wav_to_mel_spectrogram_batch(torch.from_numpy(np.stack([wav, wav[::-1].copy()])))
    assert tuple(batch.shape) == (2, mel.shape[0], 40) and np.array_equal(batch[0].numpy(), mel)
    # volume: raised to -30 dBFS when quieter, left alone when louder
    quiet = I.audio.normalize_volume(wav * 0.1, -30, increase_only=True)
    assert abs(10 * np.log10(np.mean(quiet ** 2)) + 30) < 1e-3
    assert I.audio.normalize_volume(wav * 10, -30, increase_only=True) is not None and np.array_equal(
        I.audio.normalize_volume(wav * 10, -30, increase_only=True), wav * 10)
    both = I.audio.normalize_volume_batch(torch.from_numpy(np.stack([wav * 0.1, wav * 10])), -30, increase_only=True)
    assert np.allclose(both[0].numpy(), quiet, rtol=1e-4, atol=1e-7) and torch.equal(both[1], torch.from_numpy(wav * 10))


def test_preprocess_wav_without_the_optional_packages(I):
    wav = SO.harmonic_wav(16000, 150.0, seed=2) * 0.1
    out = I.preprocess_wav(wav, trim_silence=False)
    assert out.shape == wav.shape and abs(10 * np.log10(np.mean(out ** 2)) + 30) < 1e-3
    for module, call in (("webrtcvad", lambda: I.preprocess_wav(wav)), ("librosa", lambda: I.preprocess_wav(wav, source_sr=22050, trim_silence=False)),
                         ("librosa", lambda: I.preprocess_wav("no-such-file.wav"))):
        try:
            importlib.import_module(module)
        except ImportError:
            with pytest.raises(RuntimeError, match=module):
                call()


def test_the_package_imports_as_top_level_encoder_with_torch_and_numpy_alone():
    """The notebook's binding (sys.path.append('speaker_encoder/'); from encoder import inference) in a fresh interpreter in which the
    optional packages cannot be imported; the get_embed path returns a unit-norm [256] float32 array."""
    code = """
import sys, importlib.abc
class Block(importlib.abc.MetaPathFinder):
    def find_spec(self, name, path=None, target=None):
        if name.split('.')[0] in ('librosa', 'webrtcvad', 'torchaudio', 'scipy', 'sklearn', 'matplotlib'):
            raise ImportError('blocked: ' + name)
sys.meta_path.insert(0, Block())
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from encoder import inference as spk_encoder
from encoder.model import SpeakerEncoder
torch.manual_seed(0)
torch.save({'model_state': SpeakerEncoder('cpu', 'cpu').state_dict(), 'step': 1}, sys.argv[2])
spk_encoder.load_model(sys.argv[2], device='cpu')
wav = np.sin(np.arange(40000) * 0.05).astype(np.float32) * 0.01
e = spk_encoder.embed_utterance(spk_encoder.preprocess_wav(wav, trim_silence=False))
assert e.shape == (256,) and e.dtype == np.float32 and abs(float(np.linalg.norm(e)) - 1) < 1e-5, (e.shape, e.dtype)
print('ok')
"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.check_output([sys.executable, "-c", code, os.path.join(ROOT, "speech-backbones_amd", "diffvc", "speaker_encoder"),
                                       os.path.join(d, "e.pt")], cwd=d).decode()
    assert out.strip().endswith("ok")


@pytest.mark.parametrize("seconds", [2.3, 10.0])
def test_cpu_path_of_embed_utterance(I, seconds):
    sd = SO.state("default")
    wav = I.preprocess_wav(SO.harmonic_wav(int(16000 * seconds), 150.0, seed=5), trim_silence=False)
    want, want_partials = SO.utterance_recipe(sd, wav)
    embed, partials, wave_slices = I.embed_utterance(wav, return_partials=True)
    assert embed.shape == (256,) and embed.dtype == np.float32 and partials.shape == want_partials.shape
    assert float(np.abs(embed - want).max()) <= 1e-5 and float(np.abs(partials - want_partials).max()) <= 1e-5
    assert np.array_equal(I.embed_utterance(wav), embed)
    whole = I.embed_utterance(wav, using_partials=False)
    assert float(np.abs(whole - SO.utterance_recipe(sd, wav, using_partials=False)[0]).max()) <= 1e-5


@pytest.mark.parametrize("L", [40000, 46000])
def test_cpu_path_of_embed_utterance_batch(I, L):
    """46000 samples keep a last partial that reaches beyond the waveform (padded with ones); at 40000 it is dropped."""
    sd = SO.state("default")
    wavs = torch.from_numpy(np.stack([SO.harmonic_wav(L, 120.0 + 30 * b, seed=20 + b) for b in range(3)]))
    embeds, partials, wave_slices = I.embed_utterance_batch(wavs, return_partials=True)
    assert tuple(embeds.shape) == (3, 256) and tuple(partials.shape) == (3, len(wave_slices), 256)
    assert (wave_slices[-1].stop > L) == (L == 46000)
    for b in range(3):
        want, want_partials = SO.utterance_recipe(sd, wavs[b].numpy(), pad_value=1.0)          # padded with ones
        assert float(np.abs(embeds[b].numpy() - want).max()) <= 1e-5
        assert float(np.abs(partials[b].numpy() - want_partials).max()) <= 1e-5
    if L == 46000:
        zero_padded = SO.utterance_recipe(sd, wavs[0].numpy())[0]
        assert float(np.abs(embeds[0].numpy() - zero_padded).max()) > 1e-3                       # the padding value matters
    whole = I.embed_utterance_batch(wavs, using_partials=False)
    assert float(np.abs(whole[1].numpy() - SO.utterance_recipe(sd, wavs[1].numpy(), using_partials=False)[0]).max()) <= 1e-5


def test_forward_with_a_given_state_or_autograd_runs_the_modules(I):
    m, x = I._model, SO.frames("noise", 3, 7)
    h0 = (torch.zeros(3, 3, 256), torch.zeros(3, 3, 256))
    with torch.no_grad():
        assert torch.equal(m(x, h0), m(x))
    out = m(x)
    assert out.requires_grad
    assert float((out.detach().double() - SO.reference("default", "noise", 3, 7)[1]).abs().max()) <= 1e-5


@pytest.mark.parametrize("weights", SO.WEIGHTS)
def test_numpy_step_loop_equals_nn_lstm_in_double(weights):
    """Pins gate order (i, f, g, o) and the handling of both biases independently of torch's kernel."""
    sd = SO.state(weights)
    sd["lstm.bias_ih_l0"] = sd["lstm.bias_ih_l0"] + 0.3          # a bias that is not interchangeable with the other one's value
    x = SO.frames("noise", 3, 7)
    assert float(np.abs(SO.numpy_lstm(sd, x) - SO.run_torch(sd, x, torch.float64)[0].numpy()).max()) <= 1e-12
