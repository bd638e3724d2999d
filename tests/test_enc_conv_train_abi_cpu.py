"""CPU: the Conv1d gradient entry points (csrc/conv1d_train.hip, the "gradients of one Conv1d layer" block of include/gradtts_abi.h)
are exported, declared and bound, leave the ABI version at 7, answer their host-only queries from the documented formula, and refuse bad
arguments before touching a device.

Every gtts_conv1d_pack_dgrad / gtts_conv1d_wgrad call below is made with fake non-null addresses and MUST return before anything is
dereferenced or launched: each is written against the guard it exercises."""
import ctypes
import os

import pytest

import abi_util
from abi_util import S, _fake, E_NULL, E_SHAPE, E_CONFIG, E_WORKSPACE
from conftest import ROOT

NEW = ("gtts_conv1d_pack_dgrad", "gtts_conv1d_wgrad_workspace_bytes", "gtts_conv1d_wgrad", "gtts_conv1d_wgrad_info")


def test_new_symbols_are_exported_declared_and_bound(S):
    exported = abi_util.exported(S._lib.LIB_PATH)
    declared = set(abi_util.declared())
    L = S._lib.lib()
    for name in NEW:
        assert name in exported and name in declared, name
        assert getattr(L, name).argtypes, name
    assert L.gtts_conv1d_wgrad_workspace_bytes.restype is ctypes.c_size_t
    assert L.gtts_abi_version() == 7
    assert "#define GTTS_ABI_VERSION 7" in open(os.path.join(ROOT, "include", "gradtts_abi.h")).read()
    for n in ("pack_into", "pack_dgrad", "wgrad", "wgrad_info", "wgrad_workspace_bytes"):
        assert callable(getattr(S.Conv1dOp, n))


def _wgrad(L, op, x, dy, dw, ws, nws, B, Lq, im=None, om=None, db=None):
    return L.gtts_conv1d_wgrad(op._h, x, im, dy, om, dw, db, ws, nws, B, Lq, None)


def test_wgrad_refuses_on_the_host(S):
    L = S._lib.lib()
    op = S.Conv1dOp(0, 24, 48, 3)
    x, dy, dw, ws, db = _fake(5)
    need = op.wgrad_workspace_bytes(3, 17)
    # null pointers, each in turn (the masks and db may be null: those calls get as far as the workspace check)
    assert L.gtts_conv1d_wgrad(None, x, None, dy, None, dw, None, ws, need, 3, 17, None) == E_NULL
    for k in range(4):
        args = [x, dy, dw, ws]
        args[k] = None
        assert _wgrad(L, op, args[0], args[1], args[2], args[3], need, 3, 17) == E_NULL, k
        assert b"null" in L.gtts_last_error()
    # shapes
    assert _wgrad(L, op, x, dy, dw, ws, need, 0, 17) == E_SHAPE
    assert _wgrad(L, op, x, dy, dw, ws, need, 3, 0) == E_SHAPE
    assert _wgrad(L, op, x, dy, dw, ws, need, -1, 17) == E_SHAPE
    # the 2^31-byte sample limits of gtts_conv1d_forward: cout * L * 4 and ceil(cin / 16) * 16 * L * 4
    big_out = (1 << 31) // (48 * 4) + 1
    assert _wgrad(L, op, x, dy, dw, ws, 1 << 62, 1, big_out) == E_SHAPE and b"2^31" in L.gtts_last_error()
    wide_in = S.Conv1dOp(0, 100, 8, 3)                    # 112 channels in whole chunks
    assert _wgrad(L, wide_in, x, dy, dw, ws, 1 << 62, 1, (1 << 31) // (112 * 4) + 1) == E_SHAPE
    assert op.instance(1, big_out - 2)                    # ... and just below the limit the forward is served
    # a short workspace: one byte short is refused, the exact size passes the check (and the argument checks end there: with fake
    # addresses nothing may be launched, so the passing call is not made)
    assert _wgrad(L, op, x, dy, dw, ws, need - 1, 3, 17, db=db) == E_WORKSPACE
    assert b"workspace" in L.gtts_last_error() and str(need).encode() in L.gtts_last_error()
    assert _wgrad(L, op, x, dy, dw, ws, 0, 3, 17) == E_WORKSPACE


def test_mode_1_is_refused_everywhere(S):
    L = S._lib.lib()
    up = S.Conv1dOp(1, 16, 16, 8, S=4)
    x, dy, dw, ws, w = _fake(5)
    assert _wgrad(L, up, x, dy, dw, ws, 1 << 40, 2, 16) == E_CONFIG
    assert b"mode 0" in L.gtts_last_error()
    assert L.gtts_conv1d_pack_dgrad(up._h, w, ws, None) == E_CONFIG
    assert L.gtts_conv1d_wgrad_workspace_bytes(up._h, 2, 16) == 0
    info = (ctypes.c_int * 6)()
    assert L.gtts_conv1d_wgrad_info(up._h, 2, 16, ctypes.byref(info)) == E_CONFIG
    with pytest.raises(RuntimeError):
        up.wgrad_info(2, 16)
    with pytest.raises(RuntimeError):
        up.wgrad_workspace_bytes(2, 16)


def test_pack_dgrad_and_info_refuse_null(S):
    L = S._lib.lib()
    op = S.Conv1dOp(0, 48, 24, 3)
    w, blob = _fake(2)
    assert L.gtts_conv1d_pack_dgrad(None, w, blob, None) == E_NULL
    assert L.gtts_conv1d_pack_dgrad(op._h, None, blob, None) == E_NULL
    assert L.gtts_conv1d_pack_dgrad(op._h, w, None, None) == E_NULL
    assert L.gtts_conv1d_wgrad_info(op._h, 2, 16, None) == E_NULL
    assert L.gtts_conv1d_wgrad_info(None, 2, 16, ctypes.byref((ctypes.c_int * 6)())) == E_NULL
    assert L.gtts_conv1d_wgrad_workspace_bytes(None, 2, 16) == 0
    assert L.gtts_conv1d_wgrad_workspace_bytes(op._h, 0, 16) == 0 and L.gtts_conv1d_wgrad_workspace_bytes(op._h, 2, 0) == 0
    # the dilation of the handle is honoured, not refused; the transposed handle packs into the same number of bytes as any handle
    # of its geometry
    assert S.Conv1dOp(0, 48, 24, 5, dilation=3).wgrad_info(2, 70)[3] >= 1
    assert S.Conv1dOp(0, 48, 24, 3).packed_bytes() == op.packed_bytes()


@pytest.mark.parametrize("cin,cout,K,dil", [(24, 48, 3, 1), (192, 768, 3, 1), (768, 192, 3, 1), (192, 192, 5, 1), (80, 192, 1, 1),
                                            (256, 1, 1, 1), (1, 256, 1, 1), (129, 129, 11, 1), (20, 40, 5, 3)])
def test_workspace_formula_agrees_with_info(S, cin, cout, K, dil):
    """workspace = slices * (cout * cin * K + cout) * 4; slices = max(1, min(ceil(512 / tiles), ceil(chunks / 4))) with tiles =
    ceil(cout / 64) * ceil(cin / 64) * K workgroups per slice and chunks = B * ceil(L / 64); chunks per slice = ceil(chunks / slices);
    the empty slices are those that begin at or past the last chunk."""
    op = S.Conv1dOp(0, cin, cout, K, dilation=dil)
    seen_many = False
    for B in (1, 2, 3, 5, 16):
        for Lq in (1, 17, 63, 64, 65, 190, 320, 1000):
            tr, tc, chunk, ns, per, empty = op.wgrad_info(B, Lq)
            assert (tr, tc, chunk) == (64, 64, 64)
            chunks = B * ((Lq + chunk - 1) // chunk)
            tiles = ((cout + tr - 1) // tr) * ((cin + tc - 1) // tc) * K
            assert ns == max(1, min((512 + tiles - 1) // tiles, (chunks + 3) // 4)), (B, Lq)
            assert per == (chunks + ns - 1) // ns and ns * per >= chunks
            assert empty == sum(1 for s in range(ns) if s * per >= chunks) and empty < ns
            assert op.wgrad_workspace_bytes(B, Lq) == ns * (cout * cin * K + cout) * 4
            seen_many |= ns > 1
    assert seen_many
    if (cin, cout, K) == (129, 129, 11):
        assert op.wgrad_info(5, 320)[3:] == (6, 5, 1)
