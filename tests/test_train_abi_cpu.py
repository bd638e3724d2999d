"""CPU: the training entry points that predate the PostNet ones (3x3 / 1x1 convolution forward and weight gradient, resampling
convolutions, attention core, GroupNorm + Mish, final convolution, Rezero) validate their arguments before touching a device; the
32-bit-offset guard of every weight-gradient entry point refuses exactly the shapes the Python gate `conv_size_ok` refuses; and the
workspace sizes have the documented form the regime checks of tests/test_gpu_training_shapes.py read nslice from.

Every call below is made with fake non-null addresses and MUST return before anything is dereferenced or launched: each was written
against the guard it exercises in csrc/train*.hip (a call that passed every guard would launch a kernel on those addresses)."""
import ctypes

import pytest

import wgrad_regimes as R
from abi_util import L, S, _fake, OK, E_NULL, E_SHAPE, E_CONFIG, E_WORKSPACE      # (S: the fixture L asks for)
from conftest import pkg



def _each_null(call, args, required):
    """call(*args) with each required pointer (by position) replaced by NULL, everything else valid: GTTS_E_NULL every time."""
    for k in required:
        a = list(args)
        a[k] = None
        assert call(*a) == E_NULL, (call.__name__, k)


def test_conv3x3_masked_validates(L):
    x, x1, m, om, p, b, y = _fake(7)
    f = L.gtts_conv3x3_masked
    good = (x, None, 0, m, om, p, b, y, 2, 64, 64, 80, 44, None)
    _each_null(f, good, (0, 3, 5, 6, 7))                                    # x, mask, packed, bias, y (x1 and omask are optional)
    for c0 in (0, -16, 128, 144, 24):                                       # two sources: c0 a multiple of 16 inside (0, cin)
        assert f(x, x1, c0, m, om, p, b, y, 2, 128, 64, 80, 44, None) == E_SHAPE, c0
    for B, cin, cout, H, W in ((0, 64, 64, 80, 44), (2, 0, 64, 80, 44), (2, 64, -64, 80, 44), (2, 64, 64, 0, 44), (2, 64, 64, 80, 0)):
        assert f(x, None, 0, m, om, p, b, y, B, cin, cout, H, W, None) == E_SHAPE
    for cout in (32, 96, 192, 320):                                         # cout is 64 or a multiple of 128
        assert f(x, None, 0, m, om, p, b, y, 2, 64, cout, 80, 44, None) == E_SHAPE, cout


def test_conv3x3_wgrad_validates(L):
    x, x1, m, dy, dw, db, ws = _fake(7)
    f = L.gtts_conv3x3_wgrad
    nws = L.gtts_conv3x3_wgrad_workspace_bytes(2, 128, 64, 80, 44)
    assert nws > 0
    good = (x, None, 0, m, dy, dw, db, ws, nws, 2, 128, 64, 80, 44, None)
    _each_null(f, good, (0, 3, 4, 5, 7))                                    # x, mask, dy, dw, workspace (x1 and db are optional)
    # the c0 rule: with a second source, c0 is a multiple of 64 inside (0, cin) -- whole 64-channel tiles lie in one source
    for c0 in (0, -64, 128, 192, 32, 96, 16):
        assert f(x, x1, c0, m, dy, dw, db, ws, nws, 2, 128, 64, 80, 44, None) == E_SHAPE, c0
    # ... a good c0 gets past it (to the workspace check), and without a second source c0 is not looked at
    assert f(x, x1, 64, m, dy, dw, db, ws, nws - 4, 2, 128, 64, 80, 44, None) == E_WORKSPACE
    assert f(x, None, 33, m, dy, dw, db, ws, nws - 4, 2, 128, 64, 80, 44, None) == E_WORKSPACE
    for B, cin, cout, H, W in ((0, 64, 64, 80, 44), (2, 0, 64, 80, 44), (2, 64, 0, 80, 44), (2, 64, 64, -1, 44), (2, 64, 64, 80, 0),
                               (2, 96, 64, 80, 44), (2, 64, 32, 80, 44), (2, 3, 64, 80, 44)):
        assert f(x, None, 0, m, dy, dw, db, ws, nws, B, cin, cout, H, W, None) == E_SHAPE, (B, cin, cout, H, W)
    assert f(x, None, 0, m, dy, dw, db, ws, 0, 2, 128, 64, 80, 44, None) == E_WORKSPACE
    assert f(x, None, 0, m, dy, dw, db, ws, nws - 4, 2, 128, 64, 80, 44, None) == E_WORKSPACE
    assert b"workspace too small" in L.gtts_last_error()


def test_superseded_spellings_are_gone(L):
    """One exported name per op: the suffixed spellings that the full-signature entry points replaced are not in the library."""
    for name, suffixes in (("gtts_conv3x3_masked", ("2", "3")), ("gtts_conv3x3_wgrad", ("_tiled", "_tiled2")),
                           ("gtts_gn_mish_forward", ("_tb",)), ("gtts_gn_mish_backward", ("_tb",))):
        assert hasattr(L, name), name
        for suffix in suffixes:
            assert not hasattr(L, name + suffix), name + suffix


def test_conv1x1_masked_and_wgrad_validate(L):
    x, m, p, b, y = _fake(5)
    f = L.gtts_conv1x1_masked
    _each_null(f, (x, m, p, b, y, 2, 64, 384, 80, 44, None), (0, 1, 2, 3, 4))
    for B, cin, cout, H, W in ((0, 64, 128, 80, 44), (2, -1, 128, 80, 44), (2, 64, 0, 80, 44), (2, 64, 128, 0, 44), (2, 64, 128, 80, -3)):
        assert f(x, m, p, b, y, B, cin, cout, H, W, None) == E_SHAPE
    for cout in (32, 96, 192):
        assert f(x, m, p, b, y, 2, 64, cout, 80, 44, None) == E_SHAPE, cout
    x, m, dy, dw, db, ws = _fake(6)
    f = L.gtts_conv1x1_wgrad
    nws = L.gtts_conv1x1_wgrad_workspace_bytes(2, 64, 384, 80, 44)
    assert nws > 0
    _each_null(f, (x, m, dy, dw, db, ws, nws, 2, 64, 384, 80, 44, None), (0, 2, 3, 5))      # x, dy, dw, workspace (mask, db optional)
    for B, cin, cout, H, W in ((0, 64, 384, 80, 44), (2, 0, 384, 80, 44), (2, 64, 0, 80, 44), (2, 64, 384, 0, 44), (2, 64, 384, 80, 0),
                               (2, 96, 384, 80, 44), (2, 64, 100, 80, 44), (2, 2, 64, 80, 44)):
        assert f(x, m, dy, dw, db, ws, nws, B, cin, cout, H, W, None) == E_SHAPE, (B, cin, cout, H, W)
    assert f(x, None, dy, dw, None, ws, nws - 4, 2, 64, 384, 80, 44, None) == E_WORKSPACE     # (no mask, no bias: to_qkv)
    assert f(x, m, dy, dw, db, ws, 0, 2, 64, 384, 80, 44, None) == E_WORKSPACE


def test_conv_resample_validates(L):
    x, m, p, b, y = _fake(5)
    f = L.gtts_conv_resample
    for up in (0, 1):
        _each_null(f, (x, m, p, b, y, 2, 64, 64, 80, 44, up, None), (0, 1, 2, 3, 4))
        for B, cin, cout, H, W in ((0, 64, 64, 80, 44), (2, 0, 64, 80, 44), (2, 64, 0, 80, 44), (2, 64, 64, 0, 44), (2, 64, 64, 80, -2)):
            assert f(x, m, p, b, y, B, cin, cout, H, W, up, None) == E_SHAPE
        for cin, cout in ((24, 64), (64, 96), (64, 192), (8, 128)):         # cin a multiple of 16, cout 64 or a multiple of 128
            assert f(x, m, p, b, y, 2, cin, cout, 80, 44, up, None) == E_SHAPE, (cin, cout, up)
    for H, W in ((79, 44), (80, 43), (5, 7)):                               # Downsample halves both: even H and W
        assert f(x, m, p, b, y, 2, 64, 64, H, W, 0, None) == E_SHAPE, (H, W)


def test_conv_train_kernel_name_validates(L):
    """Host only: the entry point's own shape checks, then the launching dispatch describing itself -- no pointer but the buffer."""
    f = L.gtts_conv_train_kernel_name
    buf = ctypes.create_string_buffer(256)
    assert f(0, 2, 64, 0, 64, 80, 44, 0, None, 256) == E_NULL and f(0, 2, 64, 0, 64, 80, 44, 0, buf, 0) == E_NULL
    for kind in (-1, 4):
        assert f(kind, 2, 64, 0, 64, 80, 44, 0, buf, 256) == E_CONFIG, kind
    for kind in (1, 2, 3):                                                  # two sources: the 3x3 convolution only
        assert f(kind, 2, 128, 64, 64, 80, 44, 0, buf, 256) == E_CONFIG, kind
    for c0 in (-16, 144, 24):                                               # c0 a multiple of 16 inside (0, cin)
        assert f(0, 2, 128, c0, 64, 80, 44, 0, buf, 256) == E_SHAPE, c0
    for kind in (0, 1, 2, 3):                                               # what the entry points refuse
        for B, cin, cout, H, W in ((0, 64, 64, 80, 44), (2, 0, 64, 80, 44), (2, 64, -64, 80, 44), (2, 64, 64, 0, 44), (2, 64, 64, 80, 0)):
            assert f(kind, B, cin, 0, cout, H, W, 0, buf, 256) == E_SHAPE, (kind, B, cin, cout, H, W)
    for kind in (0, 1, 3):
        for cout in (32, 96, 192):
            assert f(kind, 2, 64, 0, cout, 80, 44, 1, buf, 256) == E_SHAPE, (kind, cout)
    assert f(2, 2, 96, 0, 64, 80, 44, 0, buf, 256) == E_CONFIG and f(2, 2, 64, 0, 32, 80, 44, 0, buf, 256) == E_CONFIG     # 7x7: whole 64-channel tiles
    assert f(2, 4096, 64, 0, 64, 80, 172, 0, buf, 256) == E_SHAPE                                                        # ... below 2^29 elements
    assert f(3, 2, 24, 0, 64, 80, 44, 0, buf, 256) == E_SHAPE and f(3, 2, 64, 0, 64, 79, 44, 0, buf, 256) == E_SHAPE     # Downsample: cin % 16, even H
    assert f(3, 2, 64, 0, 64, 79, 43, 1, buf, 256) == OK and buf.value == b"gtts::conv_up4_kernel"                        # (Upsample takes odd sizes)
    assert f(0, 2, 64, 0, 64, 80, 44, 0, buf, 8) == E_WORKSPACE and buf.value == b""                                      # the name does not fit
    assert f(0, 2, 64, 0, 64, 80, 44, 0, buf, 256) == OK and buf.value.startswith(b"gtts::conv_mfma_kernel<0, ")
    assert f(0, 2, 128, 64, 64, 80, 44, 0, buf, 256) == OK and f(0, 2, 64, 64, 64, 80, 44, 0, buf, 256) == OK             # c0 = cin: one source
    assert f(1, 2, 3, 0, 64, 80, 44, 0, buf, 256) == OK and buf.value.endswith(b"2, 0, float, 2, 0>")                     # ragged channels: FULLC = 0


def test_attention_core_validates(L):
    qkv, out, ctx, stat, scr, dout, dqkv, dctx, rdot = _fake(9)
    f, g = L.gtts_attn_train_forward, L.gtts_attn_train_backward
    _each_null(f, (qkv, out, ctx, stat, scr, 2, 3520, None), range(5))
    _each_null(g, (qkv, dout, ctx, stat, dqkv, dctx, rdot, scr, 2, 3520, None), range(8))
    for B, N in ((0, 3520), (-2, 3520), (2, 0), (2, -64)):
        assert f(qkv, out, ctx, stat, scr, B, N, None) == E_SHAPE
        assert g(qkv, dout, ctx, stat, dqkv, dctx, rdot, scr, B, N, None) == E_SHAPE
        assert L.gtts_attn_train_scratch_floats(B, N) == 0
    # one record (32 x 32 context partial, 32 row maxima, 32 row sums) per (sample, head, 512-pixel slice)
    for B, N, ns in ((2, 3520, 7), (16, 80 * 172, 27), (1, 512, 1), (1, 513, 2), (3, 150, 1)):
        assert L.gtts_attn_train_scratch_floats(B, N) == B * 4 * ns * (32 * 32 + 64), (B, N)


def test_gn_mish_validates(L):
    y, ga, be, m, tb, out, st, dout, dy, dg, db, dtb, scr = _fake(13)
    f, g = L.gtts_gn_mish_forward, L.gtts_gn_mish_backward
    _each_null(f, (y, ga, be, m, tb, out, st, 2, 64, 80, 44, 8, 1e-5, None), (0, 1, 2, 3, 5, 6))          # (tb optional)
    _each_null(g, (dout, y, ga, be, m, st, dy, dg, db, dtb, scr, 2, 64, 80, 44, 8, None), (0, 1, 2, 3, 4, 5, 6, 7, 8, 10))   # (dtb optional)
    bad = ((0, 64, 80, 44, 8), (2, 0, 80, 44, 8), (2, 64, 0, 44, 8), (2, 64, 80, -1, 8), (2, 64, 80, 44, 0), (2, 64, 80, 44, -8),
           (2, 60, 80, 44, 8), (2, 64, 80, 44, 7), (1, 64, 32768, 32768, 8))                                # (H * W reaches 2^30)
    for B, C, H, W, groups in bad:
        assert f(y, ga, be, m, None, out, st, B, C, H, W, groups, 1e-5, None) == E_SHAPE, (B, C, H, W, groups)
        assert g(dout, y, ga, be, m, st, dy, dg, db, None, scr, B, C, H, W, groups, None) == E_SHAPE, (B, C, H, W, groups)
    assert L.gtts_gn_mish_stats_floats(0, 8) == 0 and L.gtts_gn_mish_stats_floats(2, 0) == 0
    assert L.gtts_gn_mish_stats_floats(16, 8) >= 16 * 8 * 2                 # the (mean, rstd) pairs, then reduction scratch
    assert L.gtts_gn_mish_scratch_bytes(0, 64) == 0 and L.gtts_gn_mish_scratch_bytes(2, -1) == 0
    assert L.gtts_gn_mish_scratch_bytes(16, 64) >= (16 * 64 * 2 + 16 * 8 * 2) * 4       # [B][C][2] sums + [B][groups][2] coefficients


def test_final_conv_validates(L):
    x, w, b, m, out, dout, dx, dw, db, scr = _fake(10)
    f, g = L.gtts_final_conv_forward, L.gtts_final_conv_backward
    _each_null(f, (x, w, b, m, out, 2, 64, 80, 44, None), range(5))
    _each_null(g, (x, w, m, dout, dx, dw, db, scr, 2, 64, 80, 44, None), range(8))
    for B, C, H, W in ((0, 64, 80, 44), (2, 0, 80, 44), (2, 64, -80, 44), (2, 64, 80, 0)):
        assert f(x, w, b, m, out, B, C, H, W, None) == E_SHAPE
        assert g(x, w, m, dout, dx, dw, db, scr, B, C, H, W, None) == E_SHAPE
        assert L.gtts_final_conv_scratch_floats(B, C, H, W) == 0
    assert g(x, w, m, dout, dx, dw, db, scr, 2, 1025, 80, 44, None) == E_SHAPE          # the per-block sums of C + 1 values live in LDS
    assert L.gtts_final_conv_scratch_floats(16, 64, 80, 172) == 16 * ((80 * 172 + 255) // 256) * 65


def test_rezero_validates(L):
    f_, x, g_, y, dy, df, dg, scr = _fake(8)
    f, g = L.gtts_rezero_forward, L.gtts_rezero_backward
    _each_null(f, (f_, x, g_, y, 1024, None), range(4))
    _each_null(g, (dy, f_, g_, df, dg, scr, 1024, None), range(6))
    for n in (0, 1, 2, 3, 1023, 4 * 1000 + 2):                              # float4 passes: a positive multiple of 4
        assert f(f_, x, g_, y, n, None) == E_SHAPE, n
        assert g(dy, f_, g_, df, dg, scr, n, None) == E_SHAPE, n
    # one fp64 partial per workgroup of 256 float4 lanes; the grid stops growing at 2048 workgroups (2 097 152 elements), beyond which
    # every workgroup walks the tensor in grid strides: B = 16, 64 channels of 80 x 172 take ceil(14 090 240 / 2 097 152) = 7 passes
    for n, blocks in ((4, 1), (1024, 1), (1028, 2), (2 * 64 * 80 * 44, 440), (2048 * 1024, 2048), (2048 * 1024 + 4, 2048),
                      (16 * 64 * 80 * 172, 2048)):
        assert L.gtts_rezero_scratch_bytes(n) == blocks * 8, n


# ---- the 32-bit byte offsets of the staging loads: (int)((((size_t)b * C + c) * HW + p) * 4) includes the batch index, so a call is
# addressable iff B * max(cin, cout) * H * W * 4 < 2^31.  The Python gate (conv_size_ok, which every *_supported(shape=...) consults)
# and the C guard of each weight-gradient entry point -- the drop-in boundary for a caller that does not go through Python -- must draw
# the line at the same place: shapes on both sides of B * C * H * W = 2^29, among them ones that only B pushes over.
SIZE_GRID = [
    # B, cin, cout, H, W
    (128, 128, 128, 128, 255), (128, 128, 128, 128, 256), (127, 128, 128, 128, 256), (129, 128, 128, 128, 255),
    (819, 64, 64, 80, 128), (820, 64, 64, 80, 128), (1024, 64, 64, 80, 128), (4096, 64, 64, 80, 172),      # only B is large
    (409, 128, 128, 80, 128), (410, 128, 128, 80, 128), (1024, 128, 128, 80, 128),
    (1, 64, 64, 2048, 2048), (2, 64, 64, 2048, 2048), (3, 64, 64, 2048, 2048), (4, 64, 64, 2048, 2048),     # (2, ...): exactly 2^29
    (1, 512, 512, 1024, 1023), (1, 512, 512, 1024, 1024), (2, 512, 512, 1024, 512), (2, 512, 512, 1023, 512),
    (64, 64, 64, 256, 256), (64, 64, 128, 256, 256), (64, 128, 64, 256, 256), (32, 128, 64, 256, 511), (32, 64, 128, 512, 256),
    (16, 64, 64, 80, 172), (128, 128, 128, 80, 128), (32, 256, 256, 80, 128), (1, 64, 64, 1, 1),            # training shapes: all fine
]


def test_size_grid_straddles_the_limit():
    n = [B * max(ci, co) * H * W for B, ci, co, H, W in SIZE_GRID]
    assert sum(v < 2 ** 29 for v in n) >= 10 and sum(v >= 2 ** 29 for v in n) >= 10 and 2 ** 29 in n and 2 ** 29 - 128 * 128 * 128 in n
    # ones that only the batch pushes over: one sample alone is far below the limit
    assert sum(1 for (B, ci, co, H, W), v in zip(SIZE_GRID, n) if v >= 2 ** 29 and max(ci, co) * H * W < 2 ** 24) >= 4


@pytest.mark.parametrize("kind", ["3x3", "1x1", "7x7"])
def test_c_size_guard_agrees_with_python_gate(L, kind):
    lib = pkg()._lib
    x, x1, m, dy, dw, db, ws = _fake(7)
    supported = {"3x3": lib.conv3x3_supported, "1x1": lib.conv1x1_supported, "7x7": lib.conv7x7_supported}[kind]
    for B, cin, cout, H, W in SIZE_GRID:
        ok = lib.conv_size_ok(B, cin, cout, H, W)
        assert ok == (B * max(cin, cout) * H * W < 2 ** 29)
        assert supported(cin, cout, need_dgrad=True, shape=(B, H, W)) == ok, (kind, B, cin, cout, H, W)
        assert supported(cin, cout, need_dgrad=True), (kind, cin, cout)     # (so it is the size, not the channel counts, that decides)
        # workspace_bytes = 0: a shape the size guard lets through stops at the workspace check, one step before the launch
        if kind == "3x3":
            rc = [L.gtts_conv3x3_wgrad(x, None, 0, m, dy, dw, db, ws, 0, B, cin, cout, H, W, None)]
            if cin >= 128:
                rc.append(L.gtts_conv3x3_wgrad(x, x1, 64, m, dy, dw, db, ws, 0, B, cin, cout, H, W, None))
        elif kind == "1x1":
            rc = [L.gtts_conv1x1_wgrad(x, m, dy, dw, db, ws, 0, B, cin, cout, H, W, None),
                  L.gtts_conv1x1_wgrad(x, None, dy, dw, None, ws, 0, B, cin, cout, H, W, None)]
        else:
            rc = [L.gtts_conv7x7_wgrad(x, m, dy, dw, db, ws, 0, B, cin, cout, H, W, None)]
            if not ok:                  # (the forward / data-gradient entry point has no workspace check to stop at: refused shapes only)
                rc.append(L.gtts_conv7x7_masked(x, m, None, ws, db, dw, B, cin, cout, H, W, None))
        for r in rc:
            assert r == (E_WORKSPACE if ok else E_SHAPE), (kind, B, cin, cout, H, W, ok, rc)
        if not ok:
            assert b"too large" in L.gtts_last_error(), (kind, L.gtts_last_error())


WS_SHAPES = [(2, 64, 64, 80, 64), (1, 128, 256, 20, 44), (3, 256, 128, 10, 17), (1, 64, 64, 5, 37), (1, 64, 64, 2, 32), (1, 64, 64, 1, 1),
             (16, 64, 64, 80, 172), (16, 128, 64, 80, 172), (16, 64, 128, 40, 86), (16, 512, 128, 20, 43), (16, 64, 384, 80, 172),
             (5, 128, 128, 40, 86), (4, 64, 64, 80, 172), (32, 64, 64, 80, 128), (128, 128, 128, 80, 128), (3, 64, 64, 80, 45)]


@pytest.mark.parametrize("kind", ["3x3", "1x1", "7x7"])
def test_wgrad_workspace_formula(L, kind):
    """workspace_bytes = (nslice * tiles * taps * 4096 + nslice * cout) * 4 with 1 <= nslice <= ceil(nchunk / 4): one partial tile per
    (slice, 64 x 64 tile, tap) and one bias partial per (slice, cout), at least four chunks per workgroup; 0 for shapes the entry point
    refuses."""
    for B, cin, cout, H, W in WS_SHAPES:
        r = R.regime(L, kind, B, cin, cout, H, W)               # (asserts the divisibility and the bounds on nslice)
        tiles = (cin // 64) * (cout // 64)
        assert R.workspace_bytes(L, kind, B, cin, cout, H, W) == (r["nslice"] * tiles * R.TAPS[kind] * 4096 + r["nslice"] * cout) * 4
        assert r["per"] * r["nslice"] >= r["nchunk"] and 0 <= r["empty"] < r["nslice"]
        if r["nchunk"] <= 4:
            assert r["nslice"] == 1
    for B, cin, cout, H, W in ((2, 96, 64, 80, 44), (2, 64, 100, 80, 44), (2, 3, 64, 80, 44), (2, 0, 64, 80, 44), (2, 64, -64, 80, 44),
                               (0, 64, 64, 80, 44), (2, 64, 64, 0, 44), (2, 64, 64, 80, -1), (2, 32, 32, 80, 44)):
        assert R.workspace_bytes(L, kind, B, cin, cout, H, W) == 0, (kind, B, cin, cout, H, W)
