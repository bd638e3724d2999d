"""CPU: the training entry points of the encoders' two fp32 VALU ops (csrc/enc_train.hip, the "ABI 7 (additive)" block of
include/gradtts_abi.h) are exported and declared, leave the ABI version at 7, answer their host-only queries from the documented LDS
sizes, and refuse bad arguments before touching a device.

Every gtts_enc_attention_train_* / gtts_enc_layernorm_backward call below is made with fake non-null addresses and MUST return before
anything is dereferenced or launched: each is written against the guard it exercises."""
import ctypes
import os

import pytest

import abi_util
from abi_util import S, _fake, E_NULL, E_SHAPE, E_CONFIG
from conftest import ROOT

LDS = 160 * 1024
NEW = ("gtts_enc_attention_train_ok", "gtts_enc_attention_train_scratch_bytes", "gtts_enc_attention_train_forward",
       "gtts_enc_attention_train_backward", "gtts_enc_layernorm_backward_scratch_floats", "gtts_enc_layernorm_backward")


def lds_floats(dk, window, L):
    """(forward, query-tiled backward, key-tiled backward) dynamic LDS in floats, as include/gradtts_abi.h states them."""
    R = 2 * window + 1 if window > 0 else 0
    LP = (L + 63) // 64 * 64
    return 16 * dk + 16 * R + 16 * LP + 16, 16 * dk + 16 * R + 16 * LP + 32, 288 * dk + 32 * R + 2112


def expected_ok(C, heads, window, L):
    if C < 1 or heads < 1 or C % heads or window < 0 or L < 1:
        return 0
    return int(all(4 * f <= LDS for f in lds_floats(C // heads, window, L)))


def test_new_symbols_are_exported_declared_and_bound(S):
    exported = abi_util.exported(S._lib.LIB_PATH)
    declared = set(abi_util.declared())
    L = S._lib.lib()
    for name in NEW:
        assert name in exported and name in declared, name
        assert getattr(L, name).argtypes, name                    # the binding declares its arguments
    assert L.gtts_enc_attention_train_scratch_bytes.restype is ctypes.c_size_t
    assert L.gtts_enc_layernorm_backward_scratch_floats.restype is ctypes.c_size_t
    assert L.gtts_abi_version() == 7
    hdr = open(os.path.join(ROOT, "include", "gradtts_abi.h")).read()
    assert "#define GTTS_ABI_VERSION 7" in hdr and "ABI 7 (additive): TRAINING of the same two ops" in hdr
    for n in ("enc_attention_train_ok", "enc_attention_train_forward", "enc_attention_train_backward", "enc_layernorm_backward"):
        assert callable(getattr(S, n))


def test_train_ok_at_and_past_its_limit(S):
    ok = S.enc_attention_train_ok
    # what the issue asks for: every dk <= 96, window <= 7, L <= 2048
    for dk in (4, 10, 48, 96):
        for heads in (1, 2, 8):
            for window in (0, 1, 4, 7):
                for L in (1, 17, 180, 1024, 2048):
                    assert ok(dk * heads, heads, window, L) == 1 == expected_ok(dk * heads, heads, window, L), (dk, heads, window, L)
    # the defaults: the query-tiled backward fills the LDS last at L = 2432 (LP = 2432), refused from 2433 on
    assert 4 * lds_floats(96, 4, 2432)[1] <= LDS < 4 * lds_floats(96, 4, 2433)[1]
    got = [ok(192, 2, 4, L) for L in range(1, 2600)]
    assert got == [expected_ok(192, 2, 4, L) for L in range(1, 2600)]
    assert got[2432 - 1] == 1 and got[2433 - 1] == 0 and set(got[:2432]) == {1} and set(got[2432:]) == {0}
    # the head width: the key-tiled backward holds four [dk][64] tiles, whatever the length
    last = max(dk for dk in range(1, 400) if 4 * lds_floats(dk, 4, 1)[2] <= LDS)
    assert ok(last, 1, 4, 1) == 1 and ok(last + 1, 1, 4, 1) == 0 and 96 < last < 192
    assert ok(192, 1, 4, 17) == 0 and ok(192, 2, 4, 17) == 1
    for C, heads, window in ((192, 2, 7), (192, 2, 8), (80, 8, 4), (48, 1, 0), (96, 4, 40)):
        for L in (1, 64, 65, 2368, 2369, 2432, 2433, 2496, 2497, 2560, 5000):
            assert ok(C, heads, window, L) == expected_ok(C, heads, window, L), (C, heads, window, L)
    for bad in ((0, 1, 4, 10), (-192, 2, 4, 10), (192, 0, 4, 10), (192, -2, 4, 10), (100, 3, 4, 10), (192, 2, -1, 10), (192, 2, 4, 0),
                (192, 2, 4, -3), (192, 2, 4, 1 << 30), (192, 2, 1 << 30, 10)):
        assert S._lib.lib().gtts_enc_attention_train_ok(*bad) == 0, bad


def test_scratch_queries_are_monotone_and_zero_for_refused_shapes(S):
    L_ = S._lib.lib()
    att, lnf = L_.gtts_enc_attention_train_scratch_bytes, L_.gtts_enc_layernorm_backward_scratch_floats
    base = att(2, 192, 100, 2, 4)
    # delta [B H L] + two band tensors [B H 9 L] + partials [min(B H, 32)][2][9][96], in bytes
    assert base == 4 * (4 * 100 + 2 * 4 * 9 * 100 + 4 * 2 * 9 * 96)
    assert att(2, 192, 100, 2, 0) == 4 * 4 * 100
    prev = 0
    for Lx in range(1, 400, 7):
        cur = att(2, 192, Lx, 2, 4)
        assert cur > prev
        prev = cur
    assert att(3, 192, 100, 2, 4) > base and att(2, 192, 100, 2, 5) > base and att(64, 192, 100, 2, 4) > att(16, 192, 100, 2, 4)
    for bad in ((0, 192, 100, 2, 4), (2, 192, 0, 2, 4), (2, 192, 2433, 2, 4), (2, 100, 10, 3, 4), (2, 192, 10, 2, -1), (65536, 192, 10, 2, 4),
                (2, 192, 17, 1, 4)):
        assert att(*bad) == 0, bad
    assert lnf(2, 20, 17) == 2 * 2 * 2 * 20 and lnf(2, 20, 16) == 2 * 1 * 2 * 20 and lnf(1, 1, 1) == 2
    assert lnf(3, 20, 17) > lnf(2, 20, 17) and lnf(2, 21, 17) > lnf(2, 20, 17) and lnf(2, 20, 33) > lnf(2, 20, 17)
    for bad in ((0, 20, 17), (2, 0, 17), (2, 20, 0), (-1, 20, 17), (65536, 20, 17)):
        assert lnf(*bad) == 0, bad


def test_attention_train_forward_refuses_before_launching(S):
    lib = S._lib.lib()
    q, k, v, mask, ek, ev, drop, out, stat = _fake(9)

    def fwd(q=q, k=k, v=v, mask=mask, ek=ek, ev=ev, drop=drop, out=out, stat=stat, B=2, C=192, L=100, heads=2, window=4):
        return lib.gtts_enc_attention_train_forward(q, k, v, mask, ek, ev, drop, out, stat, B, C, L, heads, window, None)
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(mask=None), dict(out=None), dict(stat=None), dict(ek=None), dict(ev=None)):
        assert fwd(**kw) == E_NULL, kw
        assert b"gtts_enc_attention_train_forward" in lib.gtts_last_error()
    # drop is optional, and window 0 takes no embeddings: such calls get as far as the shape check
    assert fwd(drop=None, B=0) == E_SHAPE and fwd(ek=None, ev=None, window=0, L=0) == E_SHAPE
    for kw in (dict(B=0), dict(B=-2), dict(L=0), dict(L=-100), dict(B=65536), dict(C=65536 * 4, heads=65536)):
        assert fwd(**kw) == E_SHAPE, kw
    for kw in (dict(C=0), dict(C=-192), dict(heads=0), dict(heads=-2), dict(C=100, heads=3), dict(window=-1)):
        assert fwd(**kw) == E_CONFIG, kw
    assert fwd(L=2433) == E_SHAPE and b"too long" in lib.gtts_last_error()
    assert fwd(L=1 << 30) == E_SHAPE
    assert fwd(heads=1) == E_CONFIG and b"head width" in lib.gtts_last_error()              # dk = 192
    assert fwd(q=None, B=0, C=0) == E_NULL and fwd(B=0, C=0) == E_SHAPE                       # pointers, then the shape, then the configuration


def test_attention_train_backward_refuses_before_launching(S):
    lib = S._lib.lib()
    names = ("q", "k", "v", "mask", "ek", "ev", "drop", "stat", "dout", "dq", "dk", "dv", "dek", "dev", "scratch")
    good = dict(zip(names, _fake(15)))

    def bwd(B=2, C=192, L=100, heads=2, window=4, **kw):
        a = dict(good, **kw)
        return lib.gtts_enc_attention_train_backward(*[a[n] for n in names], B, C, L, heads, window, None)
    for n in names:
        if n == "drop":                                   # optional: without it the call gets as far as the shape check
            assert bwd(B=0, drop=None) == E_SHAPE
            continue
        assert bwd(**{n: None}) == E_NULL, n
        assert b"gtts_enc_attention_train_backward" in lib.gtts_last_error()
        assert bwd(B=0, **{n: None}) == E_NULL
    # without a window none of the four embedding pointers is needed
    assert bwd(window=0, ek=None, ev=None, dek=None, dev=None, L=0) == E_SHAPE
    for kw in (dict(B=0), dict(B=-2), dict(L=0), dict(B=65536), dict(C=65536 * 4, heads=65536), dict(L=2433)):
        assert bwd(**kw) == E_SHAPE, kw
    for kw in (dict(C=0), dict(heads=0), dict(C=100, heads=3), dict(window=-1), dict(heads=1)):
        assert bwd(**kw) == E_CONFIG, kw


def test_layernorm_backward_refuses_before_launching(S):
    lib = S._lib.lib()
    names = ("dout", "a", "bres", "gamma", "beta", "am", "om", "da", "dbres", "dgamma", "dbeta", "scratch")
    good = dict(zip(names, _fake(12)))

    def ln(B=2, C=20, L=17, eps=1e-4, **kw):
        a = dict(good, **kw)
        return lib.gtts_enc_layernorm_backward(*[a[n] for n in names], B, C, L, eps, 0, 0, None)
    for n in ("dout", "a", "gamma", "beta", "da", "dgamma", "dbeta", "scratch", "dbres"):
        assert ln(**{n: None}) == E_NULL, n
        assert b"gtts_enc_layernorm_backward" in lib.gtts_last_error()
    # bres (with its gradient) and the two masks are optional: without them the call gets as far as the shape check
    for kw in (dict(bres=None), dict(bres=None, dbres=None), dict(am=None), dict(om=None)):
        assert ln(B=0, **kw) == E_SHAPE, kw
    for kw in (dict(B=0), dict(B=-1), dict(C=0), dict(L=0), dict(L=-17), dict(B=65536)):
        assert ln(**kw) == E_SHAPE, kw
        assert b"bad shape" in lib.gtts_last_error()
    for eps in (0.0, -1e-4, float("nan")):
        assert ln(eps=eps) == E_CONFIG, eps
    assert ln(a=None, B=0, eps=0.0) == E_NULL and ln(B=0, eps=0.0) == E_SHAPE


def test_training_ops_have_no_cpu_fallback(S):
    import torch
    x = torch.zeros(1, 4, 8)
    with pytest.raises(RuntimeError, match="HIP tensors"):
        S.enc_attention_train_forward(x, x, x, torch.ones(1, 8), n_heads=1, window=0)
    with pytest.raises(RuntimeError, match="HIP tensors"):
        S.enc_attention_train_backward(x, x, x, torch.ones(1, 8), None, None, None, torch.zeros(1, 1, 8, 2), x, n_heads=1, window=0)
    with pytest.raises(RuntimeError, match="HIP tensors"):
        S.enc_layernorm_backward(x, x, torch.ones(4), torch.zeros(4))
