"""CPU: the entry points of the encoder-decoder gradient path (gtts_conv_dgrad_small, gtts_diffusion_noising_backward and the alignment glue
of csrc/glue_train.hip; the "ABI 7 (additive): the encoder-decoder gradient path" block of include/gradtts_abi.h) are exported, declared
and bound, leave the ABI version at 7, and refuse bad arguments on the host.

Every call below is made with fake non-null addresses and a null stream and MUST return before anything is dereferenced or launched: each
is written against the guard it exercises.  `start` and `kept` of the gather live on the device, so a kept[b] above S cannot be refused
on the host; the kernels count it as S (tests/test_gpu_glue_train_ops.py runs that), and what the host refuses in its place is a window
longer than the frame axis, S > T."""
import ctypes

import pytest

import abi_util
from abi_util import S, _fake, E_NULL, E_SHAPE, E_CONFIG

NEW = ("gtts_conv_dgrad_small", "gtts_diffusion_noising_backward", "gtts_align_index", "gtts_duration_loss", "gtts_align_gather_partials",
       "gtts_align_gather_forward", "gtts_align_gather_backward")


def test_new_symbols_are_exported_declared_and_bound(S):
    exported = abi_util.exported(S._lib.LIB_PATH)
    hdr = open(abi_util.HEADER).read()
    declared = set(abi_util.declared())
    L = S._lib.lib()
    for name in NEW:
        assert name in exported and name in declared, name
        assert getattr(L, name).argtypes, name
        assert not name.startswith(("gtts_spk_", "gtts_fgl_", "gtts_mel_", "gtts_wav_")), name
    assert L.gtts_align_gather_partials.restype is ctypes.c_size_t
    assert L.gtts_abi_version() == 7
    assert "#define GTTS_ABI_VERSION 7" in hdr and "ABI 7 (additive): the encoder-decoder gradient path" in hdr
    for n in ("conv_dgrad_small", "diffusion_noising_backward", "align_index", "duration_loss", "align_gather", "align_gather_backward"):
        assert callable(getattr(S._lib, n)), n
    T = __import__("importlib").import_module("speech-backbones_amd.model._train_ops")
    for n in ("Noising", "DurationLoss", "AlignGather", "glue_op_counts", "reset_glue_op_counts"):
        assert hasattr(T, n), n


def test_first_layer_gates_answer_true_with_a_data_gradient(S):
    for sup in (S._lib.conv3x3_supported, S._lib.conv1x1_supported):
        for cin in (2, 3):
            for need in (False, True):
                assert sup(cin, 64, need_dgrad=need) and sup(cin, 128, need_dgrad=need, shape=(16, 80, 172))
                assert not sup(cin, 96, need_dgrad=need)                               # the same _tiles(cout) condition as without
                assert not sup(cin, 64, need_dgrad=need, shape=(1 << 14, 80, 1 << 12))   # ... and the same size condition
        assert sup(2, 64, need_dgrad=False, shape=(1, 80, 4000)) and not sup(2, 64, need_dgrad=True, shape=(1, 80, 4000))   # LDS rows
        assert not sup(4, 64, need_dgrad=True)


def test_conv_dgrad_small_refuses_before_launching(S):
    lib = S._lib.lib()
    dy, w, mask, dx = _fake(4)

    def call(dy=dy, w=w, mask=mask, dx=dx, B=2, cin=2, cout=64, H=80, W=172, k=3):
        return lib.gtts_conv_dgrad_small(dy, w, mask, dx, B, cin, cout, H, W, k, None)
    for kw in (dict(dy=None), dict(w=None), dict(mask=None), dict(dx=None)):
        assert call(**kw) == E_NULL, kw
        assert b"gtts_conv_dgrad_small" in lib.gtts_last_error()
    for kw in (dict(cin=4), dict(cin=1), dict(cin=0), dict(k=2), dict(k=5), dict(k=0), dict(cout=96), dict(cout=0), dict(cout=-64), dict(cout=32)):
        assert call(**kw) == E_CONFIG, kw
        assert b"cin must be 2 or 3" in lib.gtts_last_error()
    for kw in (dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(W=-4), dict(B=65536), dict(H=1 << 15, W=1 << 14), dict(W=2290), dict(W=1 << 20)):
        assert call(**kw) == E_SHAPE, kw
    assert call(W=2290, k=1, B=0) == E_SHAPE and call(dy=None, B=0, cin=4) == E_NULL and call(B=0, cin=4) == E_SHAPE   # pointers, shape, configuration


def test_noising_backward_refuses_before_launching(S):
    lib = S._lib.lib()
    dxt, mask, t, dx0, dmu = _fake(5)

    def call(dxt=dxt, mask=mask, t=t, dx0=dx0, dmu=dmu, B=2, F=80, T=44):
        return lib.gtts_diffusion_noising_backward(dxt, mask, t, 0.05, 20.0, dx0, dmu, B, F, T, None)
    for kw in (dict(dxt=None), dict(mask=None), dict(t=None), dict(dx0=None, dmu=None)):
        assert call(**kw) == E_NULL, kw
        assert b"gtts_diffusion_noising_backward" in lib.gtts_last_error()
    # either output alone is optional: such calls get as far as the shape check
    assert call(dx0=None, B=0) == E_SHAPE and call(dmu=None, T=0) == E_SHAPE
    for kw in (dict(B=0), dict(B=-3), dict(F=0), dict(T=0), dict(T=-44)):
        assert call(**kw) == E_SHAPE, kw


def test_alignment_glue_refuses_before_launching(S):
    lib = S._lib.lib()
    a = _fake(9)
    index = lambda p=a[0], i=a[1], d=a[2], f=a[3], B=3, tx=7, T=23: lib.gtts_align_index(p, i, d, f, B, tx, T, None)
    for k in "pidf":
        assert index(**{k: None}) == E_NULL, k
    for kw in (dict(B=0), dict(B=-1), dict(tx=0), dict(T=0), dict(T=-23), dict(T=40961), dict(B=65536)):
        assert index(**kw) == E_SHAPE, kw
    assert b"gtts_align_index" in lib.gtts_last_error()

    dl = lambda lw=a[0], d=a[1], m=a[2], p=a[3], g=a[4], B=3, tx=7: lib.gtts_duration_loss(lw, d, m, p, g, B, tx, None)
    for k in ("lw", "d", "m", "p"):
        assert dl(**{k: None}) == E_NULL, k
    assert dl(g=None, B=0) == E_SHAPE                                  # the gradient is optional
    for kw in (dict(B=0), dict(tx=0), dict(B=-2), dict(tx=-7)):
        assert dl(**kw) == E_SHAPE, kw

    names = ("mu_x", "y", "idx", "start", "kept", "y_c", "mu_y", "partials")
    good = dict(zip(names, a))

    def fwd(B=3, F=80, tx=7, T=23, S=8, **kw):
        v = dict(good, **kw)
        return lib.gtts_align_gather_forward(*[v[n] for n in names], B, F, tx, T, S, None)
    for n in names:
        assert fwd(**{n: None}) == E_NULL, n
        assert b"gtts_align_gather_forward" in lib.gtts_last_error()
    for kw in (dict(B=0), dict(B=-1), dict(F=0), dict(tx=0), dict(T=0), dict(T=-23), dict(S=0), dict(S=-8), dict(S=24), dict(B=65536)):
        assert fwd(**kw) == E_SHAPE, kw
    assert b"1 <= S <= T" in lib.gtts_last_error()
    part = lib.gtts_align_gather_partials
    assert part(3, 80, 8) == 3 * 10 * 1 and part(16, 80, 172) == 160 and part(1, 5, 257) == 2 and part(2, 81, 256) == 22
    for bad in ((0, 80, 8), (3, 0, 8), (3, 80, 0), (-1, 80, 8)):
        assert part(*bad) == 0, bad

    names = ("g_mu_y", "mu_y", "y_c", "scale", "dur", "first", "start", "kept", "dmu_x")
    good = dict(zip(names, a))

    def bwd(B=3, F=80, tx=7, S=8, **kw):
        v = dict(good, **kw)
        return lib.gtts_align_gather_backward(*[v[n] for n in names], B, F, tx, S, None)
    for n in ("dur", "first", "start", "kept", "dmu_x"):
        assert bwd(**{n: None}) == E_NULL, n
        assert b"gtts_align_gather_backward" in lib.gtts_last_error()
    assert bwd(g_mu_y=None, scale=None) == E_NULL                       # one of the two terms is needed ...
    assert bwd(mu_y=None) == E_NULL and bwd(y_c=None) == E_NULL         # ... and the prior term reads mu_y and y_c
    assert bwd(g_mu_y=None, B=0) == E_SHAPE and bwd(scale=None, mu_y=None, y_c=None, B=0) == E_SHAPE
    for kw in (dict(B=0), dict(F=0), dict(tx=0), dict(S=0), dict(S=-8), dict(B=65536)):
        assert bwd(**kw) == E_SHAPE, kw


def test_the_new_ops_have_no_cpu_fallback(S):
    import torch
    x = torch.zeros(1, 4, 8)
    L = S._lib
    for call in (lambda: L.conv_dgrad_small(torch.zeros(1, 64, 2, 2), torch.zeros(64, 2, 3, 3)),
                 lambda: L.diffusion_noising_backward(x, torch.ones(1, 8), torch.ones(1), 0.05, 20.0),
                 lambda: L.align_index(x), lambda: L.duration_loss(torch.zeros(1, 4), torch.zeros(1, 4), torch.ones(1, 4)),
                 lambda: L.align_gather(x, x, torch.zeros(1, 8, dtype=torch.int32), [0], [8], 8),
                 lambda: L.align_gather_backward(x, x, x, None, torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.int32), [0], [8])):
        with pytest.raises(RuntimeError, match="HIP tensors"):
            call()
