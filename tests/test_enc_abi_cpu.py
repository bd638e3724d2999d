"""CPU: the encoder entry points (csrc/enc.hip) decide which attention kernel serves a length, refuse what neither kernel holds, and
validate their arguments, all before touching a device.

gtts_enc_attention_path reports the decision gtts_enc_forward dispatches by (one static function in enc.hip serves both), so the GPU
cases of tests/test_gpu_utterance_shapes.py read which kernel ran from the library.  Here the hand-over and the limit are derived
from the documented LDS sizes (include/gradtts_abi.h) and the library must agree at every length around them.

Every gtts_enc_forward / gtts_enc_layernorm / gtts_enc_attention call below is made with fake non-null addresses and MUST return
before anything is dereferenced or launched: each is written against the guard it exercises (a call that passed every guard would
launch kernels on those addresses)."""
import ctypes

import pytest

from abi_util import S, _fake, OK, E_NULL, E_SHAPE, E_CONFIG, E_WORKSPACE

LDS = 160 * 1024                                    # bytes of LDS one workgroup can have on gfx950


def lds16(dk, L):
    """enc_attention16_kernel: [dk][16] queries, [16][16] relative scores, [16][roundup(L, 64)] probabilities, [4][64] output totals."""
    return (dk * 16 + 16 * 16 + 16 * ((L + 63) // 64 * 64) + 4 * 64) * 4


def lds8(dk, L):
    """enc_attention_kernel: [8][dk] queries, [8][L] probabilities."""
    return (8 * dk + 8 * L) * 4


def expected_path(C, heads, window, L):
    dk = C // heads
    if lds16(dk, L) <= LDS and dk % 4 == 0 and window <= 7:
        return 16
    return 8 if lds8(dk, L) <= LDS else 0


def test_default_configuration_hand_over_and_limit(S):
    """192 channels, 2 heads (dk 96), window 4: the 16-query kernel up to L = 2432, the 8-query kernel up to 5024, then refusal."""
    # the three edges, from the formulas alone: both kernels fill the 160 KB exactly at their last length
    assert lds16(96, 2432) == LDS and lds16(96, 2433) > LDS
    assert lds8(96, 5024) == LDS and lds8(96, 5025) > LDS
    assert [expected_path(192, 2, 4, L) for L in (1, 2432, 2433, 5024, 5025)] == [16, 16, 8, 8, 0]
    for mode in ("text", "mel"):
        enc = S.Encoder(mode)
        got = [enc.attention_path(L) for L in range(1, 5200)]
        assert got == [expected_path(192, 2, 4, L) for L in range(1, 5200)]
        assert got[2432 - 1] == 16 and got[2433 - 1] == 8 and got[5024 - 1] == 8 and got[5025 - 1] == 0
        assert set(got[:2432]) == {16} and set(got[2432:5024]) == {8} and set(got[5024:]) == {0}
        assert enc.attention_path(0) == 0 and enc.attention_path(-5) == 0 and enc.attention_path(1 << 30) == 0
    assert S._lib.lib().gtts_enc_attention_path(None, 100) == 0


@pytest.mark.parametrize("C,heads,window,want_small", [
    (192, 2, 7, 16),            # the last slot of the 16 relative scores per query (2 * 7 + 1 = 15)
    (192, 2, 8, 8),             # 17 relative positions do not fit them
    (192, 2, 0, 16),            # no relative window
    (80, 8, 4, 8),              # dk = 10: the 16-query kernel reads its queries as float4
    (96, 4, 4, 16), (96, 4, 8, 8), (144, 8, 3, 8), (48, 1, 5, 16),
])
def test_window_and_head_width_select_the_path(S, C, heads, window, want_small):
    enc = S.Encoder("mel", 0, 80, C, 4 * C, 0, heads, 2, 3, window)
    for L in (1, 7, 65, 130, 1024):
        assert enc.attention_path(L) == want_small == expected_path(C, heads, window, L), (C, heads, window, L)
    # ... and the limit follows the head width: every length around both edges
    dk = C // heads
    last16 = max([L for L in range(1, 3000) if lds16(dk, L) <= LDS]) if want_small == 16 else 0
    last8 = (LDS // 4 - 8 * dk) // 8
    assert lds8(dk, last8) <= LDS < lds8(dk, last8 + 1)
    for L in (last16, last16 + 1, last8 - 1, last8, last8 + 1, last8 + 64):
        if L > 0:
            assert enc.attention_path(L) == expected_path(C, heads, window, L), (C, heads, window, L)
    assert enc.attention_path(last8) == 8 and enc.attention_path(last8 + 1) == 0
    if last16:
        assert enc.attention_path(last16) == 16 and enc.attention_path(last16 + 1) == 8


def _forward(S, enc, packed, ids, mel, mask, mu, logw, ws, nws, B, L):
    return S._lib.lib().gtts_enc_forward(enc._h, packed, ids, mel, mask, mu, logw, ws, nws, B, L, None)


@pytest.mark.parametrize("mode", ["text", "mel"])
def test_forward_refuses_before_launching(S, mode):
    enc = S.Encoder(mode)
    lib = S._lib.lib()
    packed, ids, mel, mask, mu, logw, ws = _fake(7)
    first_refused = next(L for L in range(1, 1 << 16) if enc.attention_path(L) == 0)
    assert first_refused == 5025
    B = 2
    nws = lib.gtts_enc_workspace_bytes(enc._h, B, first_refused)
    assert nws > 0
    # the first refused length, with a workspace that is large enough: the length is what is refused
    assert _forward(S, enc, packed, ids, mel, mask, mu, logw, ws, nws, B, first_refused) == E_SHAPE
    assert b"too long" in lib.gtts_last_error()
    assert _forward(S, enc, packed, ids, mel, mask, mu, logw, ws, 1 << 40, 1, 1 << 20) == E_SHAPE
    # a short workspace, at lengths on both paths and at the refused one (the workspace is checked first)
    for L in (100, 2432, 2433, 5024, first_refused):
        need = lib.gtts_enc_workspace_bytes(enc._h, B, L)
        assert need > 0 and lib.gtts_enc_workspace_bytes(enc._h, B, L) >= 9 * B * 192 * L * 4
        for short in (0, need - 1):
            assert _forward(S, enc, packed, ids, mel, mask, mu, logw, ws, short, B, L) == E_WORKSPACE, (L, short)
        assert b"workspace too small" in lib.gtts_last_error()
    # bad B / L come before everything that depends on them
    for b, L in ((0, 100), (-1, 100), (2, 0), (2, -7)):
        assert _forward(S, enc, packed, ids, mel, mask, mu, logw, ws, 1 << 40, b, L) == E_SHAPE
        assert lib.gtts_enc_workspace_bytes(enc._h, b, L) == 0
    # each required pointer (workspace_bytes = 0: a call that got past the pointer checks stops at the workspace check)
    good = [packed, ids, mel, mask, mu, logw, ws]
    required = (0, 3, 4, 6) + ((1, 5) if mode == "text" else (2,))          # packed, x_mask, mu, workspace; ids + logw / mel
    for k in range(7):
        a = list(good)
        a[k] = None
        rc = _forward(S, enc, *a, 0, B, 100)
        assert rc == (E_NULL if k in required else E_WORKSPACE), (mode, k, rc)
    assert lib.gtts_enc_forward(None, packed, ids, mel, mask, mu, logw, ws, 0, B, 100, None) == E_NULL
    assert lib.gtts_enc_workspace_bytes(None, B, 100) == 0


def test_create_refusals(S):
    lib = S._lib.lib()
    E = S._lib.EncCfg
    h = ctypes.c_void_p()
    good = dict(mode=0, n_vocab=149, n_feats=80, channels=192, filter_channels=768, filter_channels_dp=256, n_heads=2, n_layers=6,
                kernel_size=3, window_size=4)
    order = [f for f, _ in E._fields_]

    def create(**kw):
        cfg = E(*[dict(good, **kw)[f] for f in order])
        return lib.gtts_enc_create(ctypes.byref(cfg), ctypes.byref(h))

    assert create() == OK and h.value
    lib.gtts_enc_destroy(h)
    for mode in (0, 1):
        for kw in (dict(mode=2), dict(mode=-1), dict(channels=0), dict(channels=-192), dict(n_heads=0), dict(n_heads=-2),
                   dict(n_heads=5), dict(channels=100, n_heads=3), dict(n_layers=-1), dict(kernel_size=4), dict(kernel_size=0),
                   dict(kernel_size=13), dict(window_size=-1), dict(n_feats=0), dict(n_feats=-80)):
            assert create(**dict(dict(mode=mode), **kw)) == E_CONFIG, kw
    cfg = E(*[good[f] for f in order])
    assert lib.gtts_enc_create(None, ctypes.byref(h)) == E_NULL
    assert lib.gtts_enc_create(ctypes.byref(cfg), None) == E_NULL
    # accepted edges: no window, the widest kernel, one head, no transformer layers
    for kw in (dict(window_size=0), dict(kernel_size=11), dict(kernel_size=1), dict(n_heads=1), dict(n_layers=0), dict(window_size=8)):
        assert create(**kw) == OK, kw
        lib.gtts_enc_destroy(h)
    with pytest.raises(RuntimeError):
        S.Encoder("text", window_size=-1)


# ------------------------------------------------------------------------------ the stand-alone ops: gtts_enc_layernorm / gtts_enc_attention
def test_attention_path_for_is_the_handle_query_without_a_handle(S):
    lib = S._lib.lib()
    for C, heads, window in ((192, 2, 4), (192, 2, 7), (192, 2, 8), (192, 2, 0), (80, 8, 4), (96, 4, 4), (144, 8, 3), (48, 1, 5), (96, 1, 4),
                             (4, 1, 4), (32, 8, 4)):
        enc = S.Encoder("mel", 0, 80, C, 4 * C, 0, heads, 1, 3, window)
        dk = C // heads
        last8 = (LDS // 4 - 8 * dk) // 8
        for L in list(range(1, 200)) + [1024, 2432, 2433, 2500, last8 - 1, last8, last8 + 1, 1 << 20]:
            got = S.enc_attention_path(C, heads, window, L)
            assert got == enc.attention_path(L) == expected_path(C, heads, window, L), (C, heads, window, L, got)
    assert S.enc_attention_path(96, 1, 4, 2432) == 16 and S.enc_attention_path(96, 1, 4, 2433) == 8
    assert S.enc_attention_path(96, 1, 4, 5024) == 8 and S.enc_attention_path(96, 1, 4, 5025) == 0
    for bad in ((0, 1, 4, 10), (-192, 2, 4, 10), (192, 0, 4, 10), (192, -2, 4, 10), (100, 3, 4, 10), (192, 2, -1, 10), (192, 2, 4, 0),
                (192, 2, 4, -3)):
        assert lib.gtts_enc_attention_path_for(*bad) == 0, bad


def test_layernorm_refuses_before_launching(S):
    lib = S._lib.lib()
    a, bres, gamma, beta, am, om, out = _fake(7)

    def ln(a=a, bres=bres, gamma=gamma, beta=beta, am=am, om=om, out=out, B=2, C=20, L=17, eps=1e-4):
        return lib.gtts_enc_layernorm(a, bres, gamma, beta, am, om, out, B, C, L, eps, 0, 0, None)
    for kw in (dict(a=None), dict(gamma=None), dict(beta=None), dict(out=None)):
        assert ln(**kw) == E_NULL, kw
        assert b"gtts_enc_layernorm" in lib.gtts_last_error()
    # bres and the two masks are optional: without them the call gets as far as the shape check
    for kw in (dict(bres=None), dict(am=None), dict(om=None), dict(bres=None, am=None, om=None)):
        assert ln(B=0, **kw) == E_SHAPE, kw
    for kw in (dict(B=0), dict(B=-1), dict(C=0), dict(C=-20), dict(L=0), dict(L=-17), dict(B=65536)):
        assert ln(**kw) == E_SHAPE, kw
        assert b"bad shape" in lib.gtts_last_error()
    for eps in (0.0, -1e-4, float("nan")):
        assert ln(eps=eps) == E_CONFIG, eps
    assert ln(a=None, B=0, eps=0.0) == E_NULL                       # pointers first, then the shape, then eps
    assert ln(B=0, eps=0.0) == E_SHAPE


def test_attention_refuses_before_launching(S):
    lib = S._lib.lib()
    q, k, v, mask, ek, ev, out = _fake(7)

    def att(q=q, k=k, v=v, mask=mask, ek=ek, ev=ev, out=out, B=2, C=192, L=100, heads=2, window=4, path=0):
        return lib.gtts_enc_attention(q, k, v, mask, ek, ev, out, B, C, L, heads, window, path, None)
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(mask=None), dict(out=None), dict(ek=None), dict(ev=None)):
        assert att(**kw) == E_NULL, kw
        assert b"gtts_enc_attention" in lib.gtts_last_error()
    # window 0 takes no embeddings: with both null the call gets as far as the length check
    assert att(ek=None, ev=None, window=0, L=5025) == E_SHAPE
    assert b"too long" in lib.gtts_last_error()
    for kw in (dict(B=0), dict(B=-2), dict(L=0), dict(L=-100), dict(B=65536), dict(C=65536 * 4, heads=65536)):
        assert att(**kw) == E_SHAPE, kw
    for kw in (dict(C=0), dict(C=-192), dict(heads=0), dict(heads=-2), dict(C=100, heads=3), dict(window=-1), dict(path=7), dict(path=-8),
               dict(path=1), dict(path=32)):
        assert att(**kw) == E_CONFIG, kw
    # a forced 16 where enc_attention_path's conditions do not hold: the head width, the window, the LDS
    assert att(C=80, heads=8, path=16) == E_CONFIG and b"16-query" in lib.gtts_last_error()          # dk = 10
    assert att(window=8, path=16) == E_CONFIG and b"16-query" in lib.gtts_last_error()
    assert att(C=96, heads=1, L=2433, path=16) == E_SHAPE and b"16-query" in lib.gtts_last_error()
    assert att(L=2433, path=16) == E_SHAPE
    # either kernel past its 160 KB, and the dispatch's own choice past both
    for path in (0, 8, 16):
        assert att(C=96, heads=1, L=5025, path=path) == E_SHAPE, path
        assert b"too long" in lib.gtts_last_error()
    assert att(C=96, heads=1, L=1 << 30, path=8) == E_SHAPE
    assert att(C=80, heads=8, L=(LDS // 4 - 8 * 10) // 8 + 1, path=8) == E_SHAPE


def test_stand_alone_ops_have_no_cpu_fallback(S):
    import torch
    x = torch.zeros(1, 4, 8)
    with pytest.raises(RuntimeError, match="HIP tensors"):
        S.enc_layernorm(x, torch.ones(4), torch.zeros(4))
    with pytest.raises(RuntimeError, match="HIP tensors"):
        S.enc_attention(x, x, x, torch.ones(1, 8), n_heads=1, window=0)
