"""CPU: the binding's argument rule (_in, _out) on CPU tensors, and the cap on tests/wrapper_arg_cases.py: every public function of the
binding that launches has a case, and no launch is spelled beside the one launch call."""
import inspect
import os
import re

import pytest
import torch

from conftest import pkg
from wrapper_arg_cases import CASES

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def L():
    return pkg()._lib


def test_an_input_is_refused_for_each_reason(L):
    good = torch.zeros(2, 3)
    for exc in (L.ArgumentError, ValueError, RuntimeError):                      # the decoder wrappers' type and the encoder wrappers'
        with pytest.raises(exc, match=r"op: x has shape \(2, 3\), expected \(2, 4\)"):
            L._in("op", "x", good, (2, 4), CPU)
    with pytest.raises(ValueError, match=r"op: x has 6 elements \(shape \(2, 3\)\), expected 8"):
        L._in("op", "x", good, 8, CPU)
    with pytest.raises(ValueError, match="op: x is required"):
        L._in("op", "x", None, (2, 3), CPU)
    with pytest.raises(RuntimeError, match="op: x must live on a HIP device .got meta.*no CPU fallback"):
        L._in("op", "x", torch.zeros(2, 3, device="meta"), (2, 3), CPU)
    with pytest.raises(RuntimeError, match="op: x must live on a HIP device .got cpu.*HIP tensors.*no CPU fallback"):
        L._in("op", "x", good)                                                   # the call's first tensor defines its device: a HIP one
    for strict_bad in (good.double(), torch.zeros(3, 2).t()):
        assert strict_bad.shape == (2, 3)
        with pytest.raises(RuntimeError, match="op: x must be a contiguous torch.float32 tensor"):
            L._in("op", "x", strict_bad, (2, 3), CPU, strict=True)


def test_an_accepted_input_comes_back_as_it_is(L):
    good = torch.arange(6.0).reshape(2, 3)
    for kw in (dict(), dict(strict=True), dict(optional=True)):
        assert L._in("op", "x", good, (2, 3), CPU, **kw) is good
    assert L._in("op", "x", good, 6, CPU) is good and L._in("op", "x", good, None, CPU) is good
    assert L._in("op", "x", None, (2, 3), CPU, optional=True) is None
    ids = torch.arange(4, dtype=torch.int32)
    assert L._in("op", "idx", ids, (4,), CPU, dtype=torch.int32) is ids


def test_the_coercing_mode_gives_fp32_contiguous_with_the_same_values(L):
    src = torch.arange(6, dtype=torch.float64).reshape(3, 2).t()                 # wrong dtype and wrong layout
    got = L._in("op", "x", src, (2, 3), CPU)
    assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == (2, 3) and torch.equal(got.double(), src)
    view = torch.arange(12.0).reshape(2, 6)[:, ::2]
    got = L._in("op", "x", view, (2, 3), CPU)
    assert got.is_contiguous() and torch.equal(got, view) and got.data_ptr() != view.data_ptr()


def test_an_output_is_checked_or_made(L):
    fresh = L._out("op", None, "y", (2, 3), CPU)
    assert fresh.shape == (2, 3) and fresh.dtype == torch.float32 and fresh.is_contiguous()
    assert L._out("op", {}, "y", (2,), CPU, torch.int32).dtype == torch.int32
    mine = torch.empty(2, 3)
    assert L._out("op", mine, "y", (2, 3), CPU) is mine and L._out("op", dict(y=mine), "y", (2, 3), CPU) is mine
    for wrong in (torch.empty(2, 4), torch.empty(2, 3, dtype=torch.float64), torch.empty(3, 2).t(), torch.empty(2, 3, device="meta")):
        for given in (wrong, dict(y=wrong)):
            with pytest.raises(ValueError, match="op: output y must be a contiguous torch.float32 tensor of shape .2, 3. on cpu"):
                L._out("op", given, "y", (2, 3), CPU)


def test_a_launch_needs_a_hip_device(L):
    with pytest.raises(RuntimeError, match="gtts_zero_insert2 launches on a HIP device .got cpu."):
        L._launch(CPU, "gtts_zero_insert2", torch.zeros(1), torch.zeros(1), 1, 1, 1, 1)


def _launching(L):
    """The public module-level functions of the binding that reach the launch call, directly or through a private helper of the module."""
    fns = {n: f for n, f in vars(L).items() if inspect.isfunction(f) and f.__module__ == L.__name__}
    src = {n: inspect.getsource(f) for n, f in fns.items()}
    reach = {n for n, s in src.items() if "_launch(" in s and n != "_launch"}
    while True:
        more = {n for n, s in src.items() if n not in reach and any(re.search(r"\b%s\(" % re.escape(m), s) for m in reach)}
        if not more:
            return sorted(n for n in reach if not n.startswith("_"))
        reach |= more


def test_every_launching_wrapper_has_a_case(L):
    launching = _launching(L)
    direct = [n for n, f in vars(L).items() if inspect.isfunction(f) and not n.startswith("_") and "_launch(" in inspect.getsource(f)]
    assert set(direct) <= set(launching) and len(launching) >= 53, launching
    have = {c["fn"] for c in CASES}
    assert have == set(launching), (sorted(set(launching) - have), sorted(have - set(launching)))
    for c in CASES:
        assert c["entry"].startswith("gtts_") and hasattr(L.lib(), c["entry"]), c["id"]


def test_no_launch_is_spelled_beside_the_launch_call(L):
    text = open(os.path.join(os.path.dirname(L.__file__), "_lib.py")).read()
    assert not [ln for ln in text.splitlines() if re.search(r"_check\(\s*(lib\(\)|L)\.gtts_\w+\(.*_stream\(\)", ln)]
    assert not re.findall(r"(?<![a-z])_stream\(\)", text.replace("def _stream():", "")), "no wrapper reads the stream itself"
    assert len(re.findall(r"_raw_stream\(", text)) == 3, "the stream is read where it is defined and in _launch only"
