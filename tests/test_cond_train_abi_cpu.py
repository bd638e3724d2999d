"""CPU: the entry points of the DiffVC condition path's training kernels (csrc/train_cond.hip and the time-bias entries of
csrc/train_inglu.hip; the "ABI 7 (additive): the condition path" block of include/gradtts_abi.h) are exported, declared and bound, leave
the ABI version at 7, and refuse bad arguments on the host.

Every call below is made with fake non-null addresses and a null stream and MUST return before anything is dereferenced or launched: each
is written against the guard it exercises (pointers first, then the shape, then the configuration)."""
import ctypes

import pytest

import abi_util
from abi_util import S, _fake, E_NULL, E_SHAPE, E_CONFIG, E_WORKSPACE

NEW = ("gtts_cond_field_forward", "gtts_cond_field_backward", "gtts_masked_mean_forward", "gtts_masked_mean_backward",
       "gtts_in_glu_tb_forward", "gtts_in_glu_tb_backward", "gtts_conv3x3_narrow_workspace_bytes", "gtts_conv3x3_narrow_forward",
       "gtts_conv3x3_narrow_dgrad", "gtts_conv3x3_narrow_wgrad")
BAD_SHAPES = (dict(B=0), dict(B=-1), dict(C=0), dict(C=-64), dict(H=0), dict(W=0), dict(W=-4), dict(B=65536), dict(H=1 << 16, W=1 << 15))


def test_new_symbols_are_exported_declared_and_bound(S):
    exported = abi_util.exported(S._lib.LIB_PATH)
    hdr = open(abi_util.HEADER).read()
    declared = set(abi_util.declared())
    L = S._lib.lib()
    for name in NEW:
        assert name in exported and name in declared, name
        assert getattr(L, name).argtypes, name
    assert L.gtts_abi_version() == 7
    assert "#define GTTS_ABI_VERSION 7" in hdr and "ABI 7 (additive): the condition path" in hdr
    assert L.gtts_conv3x3_narrow_workspace_bytes.restype is ctypes.c_size_t
    for n in ("cond_field", "cond_field_backward", "masked_mean", "masked_mean_backward", "in_glu_forward", "in_glu_backward",
              "conv3x3_narrow", "conv3x3_narrow_forward", "conv3x3_narrow_dgrad", "conv3x3_narrow_wgrad"):
        assert callable(getattr(S._lib, n)), n
    # one InstanceNorm + GLU wrapper pair serves both C entry pairs: the time term is an optional argument, as in gn_mish_forward / _backward
    sig = __import__("inspect").signature
    assert sig(S._lib.in_glu_forward).parameters["tb"].default is None
    assert sig(S._lib.in_glu_backward).parameters["want_dtb"].default is False
    assert not hasattr(S._lib, "in_glu_tb_forward") and not hasattr(S._lib, "in_glu_tb_backward")
    T = __import__("importlib").import_module("speech-backbones_amd.model._train_ops")
    assert sig(T.InstNormGlu.forward).parameters["tb"].default is None and not hasattr(T, "InstNormGluBias")
    for n in ("CondField", "MaskedMean", "InstNormGlu", "cond_op_counts", "reset_cond_op_counts", "COND_LEFT_ON_TORCH"):
        assert hasattr(T, n), n
    sources = __import__("importlib").import_module("speech-backbones_amd.build").SOURCES
    assert "train_cond.hip" in sources and "train_narrow.hip" in sources


def test_condition_field_refuses_before_launching(S):
    lib = S._lib.lib()
    U, mask, base, out = _fake(4)

    def fwd(U=U, mask=mask, base=base, out=out, B=2, C=64, H=80, W=36, taps=9):
        return lib.gtts_cond_field_forward(U, mask, base, out, B, C, H, W, taps, None)

    def bwd(dy=U, mask=mask, S_=out, B=2, C=64, H=80, W=36, taps=9):
        return lib.gtts_cond_field_backward(dy, mask, S_, B, C, H, W, taps, None)
    for kw in (dict(U=None), dict(mask=None), dict(out=None)):
        assert fwd(**kw) == E_NULL, kw
        assert b"gtts_cond_field_forward" in lib.gtts_last_error()
    assert fwd(base=None, B=0) == E_SHAPE                                 # the base is optional: such a call gets as far as the shape check
    for kw in (dict(dy=None), dict(mask=None), dict(S_=None)):
        assert bwd(**kw) == E_NULL, kw
        assert b"gtts_cond_field_backward" in lib.gtts_last_error()
    for call in (fwd, bwd):
        for kw in BAD_SHAPES:
            assert call(**kw) == E_SHAPE, kw
        for taps in (0, 2, 3, 8, 10, -9, 25):
            assert call(taps=taps) == E_CONFIG, taps
            assert b"taps must be 9" in lib.gtts_last_error()
        assert call(mask=None, B=0, taps=3) == E_NULL and call(B=0, taps=3) == E_SHAPE        # pointers, shape, configuration


def test_masked_mean_refuses_before_launching(S):
    lib = S._lib.lib()
    a, mask, b = _fake(3)

    def fwd(y=a, mask=mask, p=b, B=2, C=128, H=80, W=20):
        return lib.gtts_masked_mean_forward(y, mask, p, B, C, H, W, None)

    def bwd(dp=a, mask=mask, dy=b, B=2, C=128, H=80, W=20):
        return lib.gtts_masked_mean_backward(dp, mask, dy, B, C, H, W, None)
    for kw in (dict(y=None), dict(mask=None), dict(p=None)):
        assert fwd(**kw) == E_NULL, kw
        assert b"gtts_masked_mean_forward" in lib.gtts_last_error()
    for kw in (dict(dp=None), dict(mask=None), dict(dy=None)):
        assert bwd(**kw) == E_NULL, kw
        assert b"gtts_masked_mean_backward" in lib.gtts_last_error()
    for call in (fwd, bwd):
        for kw in BAD_SHAPES:
            assert call(**kw) == E_SHAPE, kw
        assert call(mask=None, B=0) == E_NULL


def test_time_bias_entries_refuse_before_launching(S):
    lib = S._lib.lib()
    a = _fake(10)
    fnames = ("y", "gamma", "beta", "tb", "out", "stats")
    bnames = ("dout", "y", "gamma", "beta", "stats", "dy", "dgamma", "dbeta", "dtb", "scratch")

    def fwd(B=2, C=32, H=80, W=20, **kw):
        v = dict(zip(fnames, a), **kw)
        return lib.gtts_in_glu_tb_forward(*[v[n] for n in fnames], B, C, H, W, 1e-5, None)

    def bwd(B=2, C=32, H=80, W=20, **kw):
        v = dict(zip(bnames, a), **kw)
        return lib.gtts_in_glu_tb_backward(*[v[n] for n in bnames], B, C, H, W, None)
    for n in fnames:
        assert fwd(**{n: None}) == E_NULL, n
        assert b"gtts_in_glu_tb_forward" in lib.gtts_last_error()
    for n in bnames:
        assert bwd(**{n: None}) == E_NULL, n
        assert b"gtts_in_glu_tb_backward" in lib.gtts_last_error()
    for call in (fwd, bwd):
        for kw in BAD_SHAPES:
            assert call(**kw) == E_SHAPE, kw
    # the entries without the bias are what they were
    assert lib.gtts_in_glu_forward(a[0], a[1], a[2], a[3], a[4], 0, 32, 80, 20, 1e-5, None) == E_SHAPE
    assert lib.gtts_in_glu_forward(None, a[1], a[2], a[3], a[4], 2, 32, 80, 20, 1e-5, None) == E_NULL


def test_narrow_convolutions_refuse_before_launching(S):
    lib = S._lib.lib()
    a = _fake(8)
    wsb = lib.gtts_conv3x3_narrow_workspace_bytes
    fn = ("x", "mask", "omask", "w", "bias", "y", "ws")
    dn = ("dy", "omask", "mask", "w", "dx", "ws")
    wn = ("x", "mask", "omask", "dy", "dw", "db", "ws")

    def call(entry, names, op, B=2, cin=32, cout=64, H=80, W=20, nbytes=None, **kw):
        v = dict(zip(names, a), **kw)
        nbytes = wsb(B, cin, cout, H, W, op) if nbytes is None else nbytes
        return entry(*[v[n] for n in names], nbytes, B, cin, cout, H, W, None)
    fwd = lambda **kw: call(lib.gtts_conv3x3_narrow_forward, fn, 0, **kw)
    dgr = lambda **kw: call(lib.gtts_conv3x3_narrow_dgrad, dn, 1, **kw)
    wgr = lambda **kw: call(lib.gtts_conv3x3_narrow_wgrad, wn, 2, **kw)
    for entry, names, optional in ((fwd, fn, ("omask",)), (dgr, dn, ("omask",)), (wgr, wn, ("omask", "db"))):
        for n in names:
            if n in optional:
                assert entry(**{n: None}, B=0) == E_SHAPE, n              # optional: such a call gets as far as the shape check
            else:
                assert entry(**{n: None}) == E_NULL, n
        assert b"gtts_conv3x3_narrow_" in lib.gtts_last_error()
        for kw in (dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(W=-4), dict(B=65536), dict(H=1 << 15, W=1 << 14)):
            assert entry(nbytes=1 << 30, **kw) == E_SHAPE, kw
        for kw in (dict(cin=2), dict(cin=64), dict(cin=0), dict(cout=32), dict(cout=96), dict(cout=256), dict(cout=0), dict(cin=16, cout=64)):
            assert entry(nbytes=1 << 30, **kw) == E_CONFIG, kw
        assert entry(nbytes=wsb(2, 32, 64, 80, 20, 2 if entry is wgr else 0) - 4) == E_WORKSPACE and entry(nbytes=0) == E_WORKSPACE
        assert b"workspace too small" in lib.gtts_last_error()
        assert entry(mask=None, B=0, cin=7) == E_NULL and entry(B=0, cin=7, nbytes=8) == E_SHAPE and entry(cin=7, nbytes=0) == E_CONFIG
    assert dgr(cin=1, nbytes=1 << 20) == E_CONFIG and b"cin must be 32" in lib.gtts_last_error()      # block11's input is data
    # workspace sizes: the re-laid-out weights; B x slices records of dw + db
    assert wsb(2, 32, 64, 80, 20, 0) == wsb(2, 32, 64, 80, 20, 1) == 9 * 32 * 64 * 4 and wsb(2, 1, 128, 3, 5, 0) == 9 * 128 * 4
    assert wsb(2, 32, 64, 80, 20, 2) == 2 * 7 * (64 * 32 * 9 + 64) * 4 and wsb(16, 32, 128, 80, 128, 2) == 16 * 16 * (128 * 32 * 9 + 128) * 4
    assert wsb(3, 1, 64, 1, 1, 2) == 3 * 1 * (64 * 9 + 64) * 4
    for bad in ((0, 32, 64, 80, 20, 0), (2, 2, 64, 80, 20, 0), (2, 32, 96, 80, 20, 2), (2, 1, 64, 80, 20, 1), (2, 32, 64, 80, 20, 3), (2, 32, 64, 0, 20, 0)):
        assert wsb(*bad) == 0, bad
    sup = S._lib.conv3x3_supported
    assert sup(32, 64) and sup(32, 128, shape=(32, 80, 128)) and sup(1, 64, need_dgrad=False) and not sup(1, 64, need_dgrad=True)
    assert not sup(32, 96) and not sup(16, 64) and not sup(1, 32, need_dgrad=False) and not sup(32, 64, shape=(1 << 14, 80, 1 << 12))


def test_the_new_ops_have_no_cpu_fallback_and_check_their_shapes(S):
    import torch
    L = S._lib
    x, m = torch.zeros(1, 4, 2, 3), torch.ones(1, 3)
    for call in (lambda: L.cond_field(torch.zeros(1, 9, 4), m, 2, x), lambda: L.cond_field_backward(x, m, 9),
                 lambda: L.masked_mean(x, m), lambda: L.masked_mean_backward(torch.zeros(1, 4), m, 2),
                 lambda: L.in_glu_forward(x, torch.ones(4), torch.zeros(4), tb=torch.zeros(1, 2)),
                 lambda: L.conv3x3_narrow_forward(torch.zeros(1, 1, 2, 3), m, torch.zeros(64, 1, 3, 3), torch.zeros(64)),
                 lambda: L.conv3x3_narrow_dgrad(torch.zeros(1, 64, 2, 3), torch.zeros(64, 32, 3, 3), m),
                 lambda: L.conv3x3_narrow_wgrad(torch.zeros(1, 32, 2, 3), m, torch.zeros(1, 64, 2, 3))):
        with pytest.raises(RuntimeError, match="HIP"):
            call()


def test_the_condition_columns_and_final_conv_are_never_left_on_torch(S):
    T = __import__("importlib").import_module("speech-backbones_amd.model._train_ops")
    assert isinstance(T.COND_LEFT_ON_TORCH, frozenset)
    assert all(len(k) == 2 and k[0] in (1, 32) and k[1] in (64, 128) for k in T.COND_LEFT_ON_TORCH), T.COND_LEFT_ON_TORCH
    T.reset_cond_op_counts()
    assert T.cond_op_counts() == (0, 0)
    T.cond_count(True)
    T.cond_count(False)
    assert T.cond_op_counts() == (1, 1)
    T.reset_cond_op_counts()
