"""CPU tests of the log-mel gradient's ABI and binding (csrc/mel_train.hip, _lib.MelPlan.backward, hifi_gan/meldataset.py): symbols,
the host-side refusals (no device is touched: every pointer handed over is a dummy the library must not follow), the binding's checks and
the torch path of the drop-in under autograd."""
import ctypes
import importlib
import re

import pytest
import torch

import mel_grad_cases as C
import mel_oracle as MO
import abi_util
from conftest import pkg

NEW = {"gtts_mel_backward", "gtts_mel_backward_workspace_bytes"}


@pytest.fixture(scope="module")
def MD():
    return importlib.import_module("speech-backbones_amd.hifi_gan.meldataset")


def test_new_symbols_are_exported_and_declared_and_the_version_stays():
    S = pkg()
    assert abi_util.exported(S._lib.LIB_PATH) >= NEW
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gradtts_abi.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header)
    assert S._lib.lib().gtts_abi_version() == 7
    assert "#define GTTS_ABI_VERSION 7" in header


def test_host_side_refusals_touch_no_device():
    S = pkg()
    L, m = S._lib.lib(), S.MelPlan(*MO.CFG1)
    h, p = m._h, ctypes.c_void_p(64)                   # p: a non-null pointer nothing may read through
    big = 1 << 40

    def call(handle=h, packed=p, wav=p, dmel=p, dwav=p, ws=p, nbytes=big, B=2, n=845):
        return L.gtts_mel_backward(handle, packed, wav, None, dmel, dwav, ws, nbytes, B, n, None)
    for kw in (dict(handle=None), dict(packed=None), dict(wav=None), dict(dmel=None), dict(dwav=None), dict(ws=None)):
        assert call(**kw) == -1                        # GTTS_E_NULL
        assert b"gtts_mel_backward: null argument" in L.gtts_last_error()
    for B in (0, -1, 65536):
        assert call(B=B) == -2 and b"B must lie in [1, 65535]" in L.gtts_last_error()
    assert call(n=384) == -2 and b"reflect" in L.gtts_last_error()             # L <= pad
    assert call(n=0x7fffffff) == -2 and b"32-bit" in L.gtts_last_error()
    wide = S.MelPlan(512, 40, 16000, 400, 512, 0, 8000)
    assert call(handle=wide._h, n=300) == -2 and b"whole frame" in L.gtts_last_error()
    need = m.backward_workspace_bytes(2, 845)
    assert need >= 2 * 3 * 1024 * 4 and need % 256 == 0
    assert call(nbytes=need - 1) == -6 and b"workspace too small" in L.gtts_last_error()   # GTTS_E_WORKSPACE
    assert L.gtts_mel_backward_workspace_bytes(None, 2, 845) == 0 and L.gtts_mel_backward_workspace_bytes(h, 0, 845) == 0
    assert L.gtts_mel_backward_workspace_bytes(h, 2, 384) == 0
    assert m.backward_workspace_bytes(16, 8192) == 16 * 32 * 1024 * 4
    with pytest.raises(RuntimeError, match="reflect"):
        m.backward_workspace_bytes(2, 384)


def test_every_configuration_the_forward_serves_has_a_backward_plan():
    """gtts_mel_create refuses nothing it accepted before, the n_fft = 2048, all-bins configuration included."""
    S = pkg()
    for cfg in C.CFGS.values():
        m = S.MelPlan(*cfg)
        assert m.backward_workspace_bytes(1, 4 * cfg[0]) == m.frames(4 * cfg[0]) * cfg[0] * 4


def test_binding_refuses_cpu_tensors_and_wrong_shapes():
    m = pkg().MelPlan(*MO.CFG1)
    y, d = MO.signal("noise", 845), torch.zeros(3, 80, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.backward(None, y, d)
    with pytest.raises(RuntimeError, match=r"\[B, L\]"):
        m.backward(None, y[0], d)
    for bad in (torch.zeros(3, 80, 4), torch.zeros(2, 80, 3), torch.zeros(3, 79, 3), torch.zeros(3, 80 * 3)):
        with pytest.raises(RuntimeError, match="dmel must be"):
            m.backward(None, y, bad)
    with pytest.raises(RuntimeError, match="reflect"):
        m.backward(None, y[:, :384], d)


def test_torch_path_differentiates_and_matches_float64(MD):
    """CPU tensors keep the torch recipe, which autograd differentiates: against the float64 reference of the catalogue."""
    case = ("cfg1", 845, None, "noise")
    r = C.reference(case)
    y = r["y"].clone().requires_grad_()
    mel = MD.mel_spectrogram(y, *MO.CFG1)
    assert mel.requires_grad and mel.grad_fn is not None
    (mel * r["dmel"]).sum().backward()
    e = C.row_error(y.grad, r["ref"])
    assert float(e.max()) <= 4 * float(r["e_ref32"].max()) + 2e-6
    # ragged rows on the torch path: gradient 0 at and beyond each length
    rag = (C.RAGGED[0], C.RAGGED[1], C.RAGGED[2], "noise")
    r = C.reference(rag)
    y = r["y"].clone().requires_grad_()
    mel, _ = MD.mel_spectrogram(y, *MO.CFG1, y_lengths=list(C.RAGGED[2]))
    (mel * r["dmel"]).sum().backward()
    assert float(C.row_error(y.grad, r["ref"]).max()) <= 4 * float(r["e_ref32"].max()) + 2e-6
    for b, n in C.rows_of(rag):
        assert bool((y.grad[b, n:] == 0).all())
