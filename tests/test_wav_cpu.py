"""CPU: the host side of the speaker encoder's waveform front end (csrc/wav.hip) -- exported symbols, the configuration struct's layout,
refusals decided before a device is touched, the packed resampling taps -- and the torch path of the drop-in encoder/audio.py against
the restatement in tests/wav_oracle.py, with one anchor that does not come from the restatement (an analytic sine)."""
import copy
import ctypes
import math
import os
import pickle
import subprocess

import numpy as np
import pytest
import torch

import wav_oracle as WO
import abi_util
from conftest import ROOT, pkg


@pytest.fixture(scope="module")
def A():
    return WO.audio()


def test_preprocess_wav_batch_needs_no_torchaudio(A, monkeypatch):
    """On a CPU tensor, in an interpreter in which torchaudio cannot be imported.  Against the oracle in float32: <= 2e-7, not bit for
    bit -- both run the same strided conv1d, but the module's kernel comes from numpy and the oracle's from torch, whose float64 sin /
    cos may differ in the last place before the rounding to fp32 (one fp32 ulp of a tap <= 0.73 times |x| <= 1 is 6e-8)."""
    monkeypatch.setitem(__import__("sys").modules, "torchaudio", None)
    with pytest.raises(ImportError):
        __import__("torchaudio")
    for L in (1, 5, 441, 442, 441 * 37 + 100):
        x = WO.wave("speechlike", L, 22050)
        got = A.resample_batch(x, 22050)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, -(-320 * L // 441))
        assert float((got - WO.resample(x, 22050, torch.float32)).abs().max()) <= 2e-7
        assert float((got.double() - WO.resample(x, 22050)).abs().max()) <= 2e-6
    L = 441 * 37 + 100
    x = 0.01 * WO.wave("speechlike", L, 22050)            # quieter than -30 dBFS: raised
    out = A.preprocess_wav_batch(x, 22050)
    assert tuple(out.shape) == (3, -(-320 * L // 441)) and out.dtype == torch.float32
    want = WO.normalize(WO.resample(x, 22050), -30, increase_only=True)
    assert float((out.double() - want).abs().max()) <= 2e-6
    assert float((10 * torch.log10(out.double().pow(2).mean(-1)) + 30).abs().max()) < 1e-3
    assert A.preprocess_wav_batch(x, 16000).shape == x.shape                             # nothing to resample
    assert A._ratio_on_kernels(22050) and A._ratio_on_kernels(44100) and not A._ratio_on_kernels(16010)      # 1601 / 1600: the torch recipe
    assert tuple(A.preprocess_wav_batch(x[:, :3000], 16010).shape) == (3, -(-1600 * 3000 // 1601))
    x64 = A.preprocess_wav_batch(x.double(), 22050)
    assert x64.dtype == torch.float64 and float((x64 - want).abs().max()) <= 1e-12


def test_wav_symbols_are_exported_and_the_abi_version_stays():
    S = pkg()
    exported = {n for n in abi_util.exported(S._lib.LIB_PATH) if n.startswith("gtts_wav_")}
    assert exported >= {"gtts_wav_" + op for op in ("create", "destroy", "resampled_length", "frames", "tiles", "span", "taps", "filterbank",
                                                    "packed_bytes", "pack", "workspace_bytes", "resample", "normalize", "powmel")}
    assert S._lib.lib().gtts_abi_version() == 7
    assert S.WavPlan is S._lib.WavPlan and S.WavPlan._family == "wav"


def test_cfg_struct_layout_matches_the_header(tmp_path):
    S = pkg()
    fields = [f[0] for f in S._lib.WavCfg._fields_]
    assert fields == ["source_sr", "sampling_rate", "n_fft", "hop_size", "n_mels", "lowpass_filter_width", "rolloff", "fmin", "fmax"]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "gradtts_abi.h"', 'int main(void) {',
            '  printf("%zu\\n", sizeof(gtts_wav_cfg));']
    prog += ['  printf("%%zu\\n", offsetof(gtts_wav_cfg, %s));' % f for f in fields]
    prog += ['  return 0; }']
    src = tmp_path / "cfg.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "cfg"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    nums = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert nums[0] == ctypes.sizeof(S._lib.WavCfg)
    assert nums[1:] == [getattr(S._lib.WavCfg, f).offset for f in fields]


def test_configurations_and_shapes_are_refused_on_the_host():
    S = pkg()
    p = S.WavPlan()
    assert (p.resampled_length(1), p.resampled_length(441), p.resampled_length(442), p.frames(201), p.frames(16000)) == (1, 320, 321, 2, 101)
    assert p.tiles(1024) == 1 and p.tiles(1025) == 2 and p.packed_bytes() > 0 and p.workspace_bytes(3, 1025) >= 3 * 2 * 4
    good = dict(source_sr=22050, sampling_rate=16000, n_fft=400, hop_size=160, n_mels=40, lowpass_filter_width=6, rolloff=0.99, fmin=0.0,
                fmax=8000.0)
    for bad in (dict(source_sr=22051), dict(source_sr=16000, sampling_rate=22051, fmax=8000.0),     # reduced rates beyond 1024
                dict(n_fft=401), dict(n_fft=62), dict(n_fft=1026), dict(hop_size=0), dict(hop_size=401), dict(n_mels=0), dict(n_mels=129),
                dict(fmin=-1.0), dict(fmin=8000.0), dict(fmax=8000.5), dict(lowpass_filter_width=0), dict(rolloff=0.0), dict(rolloff=1.5)):
        with pytest.raises(RuntimeError, match=r"\(-3\)"):
            S.WavPlan(**dict(good, **bad))
    S.WavPlan(**dict(good, n_fft=64, hop_size=64)), S.WavPlan(**dict(good, n_fft=1024, n_mels=128)), S.WavPlan(**dict(good, source_sr=1024 * 50, sampling_rate=1023 * 50, fmax=100.0))
    for call in (lambda: p.frames(200), lambda: p.frames(0), lambda: p.resampled_length(0), lambda: p.resampled_length(-3)):
        with pytest.raises(RuntimeError, match=r"\(-2\)"):
            call()
    # the compute entry points decide the same before they touch a device: the pointers below are never followed
    L, h, fake = S._lib.lib(), p._h, ctypes.c_void_p(4096)
    assert L.gtts_wav_powmel(h, fake, fake, fake, 1, 200, None) == -2 and b"reflect" in L.gtts_last_error()
    assert L.gtts_wav_powmel(h, fake, fake, fake, 0, 16000, None) == -2
    assert L.gtts_wav_powmel(h, fake, fake, fake, 1 << 15, 1 << 16, None) == -2 and b"2^31" in L.gtts_last_error()
    assert L.gtts_wav_powmel(h, fake, fake, fake, 40000, 1600 * 1000, None) == -2
    assert L.gtts_wav_resample(h, fake, fake, fake, fake, 1, 0, None) == -2
    assert L.gtts_wav_resample(h, fake, fake, fake, fake, 1 << 15, 1 << 16, None) == -2
    assert L.gtts_wav_normalize(h, fake, fake, -30.0, 1, fake, None, 0, 1, 0, None) == -2
    assert L.gtts_wav_normalize(h, fake, fake, -30.0, 1, fake, None, 0, 1 << 15, 1 << 16, None) == -2
    assert L.gtts_wav_normalize(h, fake, fake, -30.0, 3, fake, None, 0, 1, 100, None) == -3
    assert L.gtts_wav_normalize(h, fake, None, -30.0, 1, fake, fake, 4, 1, 100, None) == -6                # workspace too small
    same = S.WavPlan(**dict(good, source_sr=16000))
    assert same.resampled_length(777) == 777
    assert L.gtts_wav_resample(same._h, fake, fake, fake, fake, 1, 100, None) == -3 and b"nothing to resample" in L.gtts_last_error()
    with pytest.raises(RuntimeError, match="HIP device"):
        p.powmel(None, torch.zeros(1, 16000))
    with pytest.raises(ValueError, match="Both"):
        p.normalize(None, torch.zeros(1, 16000), -30, True, True)


@pytest.mark.parametrize("source_sr,sr", WO.RATIOS)
def test_packed_taps_keep_the_unclamped_support(source_sr, sr):
    """The kernel sums gtts_wav_span taps per phase: the stretch where the clamp does not bite.  What is left out is 0 in fp32."""
    k64, t_raw, w, o, n = WO.kernel64(source_sr, sr)
    first, taps = pkg().WavPlan(source_sr, sr, fmax=min(8000.0, sr / 2)).taps()
    assert tuple(taps.shape) == (n, WO.SPANS[(source_sr, sr)]) and tuple(first.shape) == (n,)
    k32 = k64.to(torch.float32)
    inside = t_raw.abs() < 6
    assert float(k64[~inside].abs().max()) < 2e-49 and bool((k32[~inside] == 0).all())
    full = torch.zeros_like(k32)
    for p in range(n):
        f = int(first[p])
        cnt = int(inside[p].sum())
        assert bool(inside[p, f:f + cnt].all()) and cnt <= taps.shape[1]                    # contiguous, starting at first[p]
        assert bool((taps[p, cnt:] == 0).all())
        full[p, f:f + cnt] = taps[p, :cnt]
    assert int(inside.sum(1).max()) == taps.shape[1]
    assert float((full - k32).abs().max()) <= 6e-8                                           # the same float64 formula, rounded once


def test_filterbank_is_the_modules(A):
    W = pkg().WavPlan().filterbank()
    assert tuple(W.shape) == (40, 201) and float((W - torch.from_numpy(A.mel_filterbank())).abs().max()) <= 1e-9


@pytest.mark.parametrize("f", [200.0, 1000.0, 3000.0])
def test_a_resampled_sine_is_the_sine_at_the_new_rate(A, f):
    """An anchor outside the restatement: one second of sin(2 pi f t) at 22050 Hz against the analytic sine at 16 kHz, away from the
    zero-padded ends.  The float64 formula gives 4.4e-4 to 5.3e-4 (its passband gain of 1.0004 to 1.0005)."""
    x = torch.sin(2 * math.pi * f * torch.arange(22050, dtype=torch.float64) / 22050)[None]
    want = torch.sin(2 * math.pi * f * torch.arange(16000, dtype=torch.float64) / 16000)[None]
    for got in (WO.resample(x, 22050), A.resample_batch(x, 22050), A.resample_batch(x.float(), 22050).double()):
        assert tuple(got.shape) == (1, 16000)
        assert float((got - want)[:, 50:-50].abs().max()) <= 2e-3


def test_the_oracles_power_mel_is_torch_stft():
    x = WO.wave("speechlike", 160 * 59 + 31, 16000).double()
    fb = torch.from_numpy(WO.audio().mel_filterbank()).double()
    s = torch.stft(x, n_fft=400, hop_length=160, win_length=400, window=torch.hann_window(400, dtype=torch.float64), center=True,
                   pad_mode="reflect", return_complex=True)
    want = torch.transpose(torch.matmul(fb, s.real ** 2 + s.imag ** 2), 1, 2)
    got = WO.powmel(x)
    assert tuple(got.shape) == (3, 60, 40) and float((got - want).abs().max()) == 0.0
    # and the module's torch path, in float32, against it
    mel = WO.audio().wav_to_mel_spectrogram_batch(x.float())
    assert float((mel.double() - got).abs().max()) <= 1e-5 * float(got.max())


def test_normalize_oracle_is_the_modules_recipe(A):
    x = WO.wave("harmonic", 16000, 16000)
    rows = torch.stack([0.01 * x[0], 10 * x[1], torch.zeros_like(x[2])])
    for kw in (dict(increase_only=True), dict(decrease_only=True), dict()):
        got, want = A.normalize_volume_batch(rows, -30, **kw), WO.normalize(rows, -30, dtype=torch.float32, **kw)
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))
    assert bool(torch.isnan(A.normalize_volume_batch(rows, -30, increase_only=True)[2]).all())


def test_wav_handle_copies_and_pickles_by_rebuilding():
    h = pkg().WavPlan(24000, 16000)
    first, taps = h.taps()
    for dup in (copy.deepcopy(h), pickle.loads(pickle.dumps(h))):
        assert type(dup) is type(h) and dup._h.value and dup._h.value != h._h.value and dup._kw == h._kw
        assert dup.packed_bytes() == h.packed_bytes() and torch.equal(dup.taps()[1], taps) and torch.equal(dup.taps()[0], first)
