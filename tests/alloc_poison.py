"""Fresh memory holds any bytes: the harness of tests/test_gpu_fresh_memory.py (include/gradtts_abi.h: workspace, scratch, saved-state
and output buffers may hold any bytes on entry).

The package takes every buffer it hands to the library from `torch.empty` / `torch.empty_like`, reached as attributes of `torch`.
`poisoned` replaces the two for the length of a `with` block: the replacement calls the real function and then fills the WHOLE storage of
a non-empty result on the device under test with a repeating 4-byte pattern.  `check` runs one closure once per pattern and holds every
tensor it returns to the bits of the all-zero run.  Nothing here touches the GPU at import and every function takes the device it works
on, so tests/test_alloc_poison_cpu.py proves on the CPU that the harness fills what it says and that `check` fires.

  0x00000000  the baseline: what a fresh process almost always hands out
  0xFFFFFFFF  NaN as fp32 and as both bf16 halves, -1 as int32, 0xFF in every fp8 byte
  0x7F800000  +Inf
  0xFF7FFFFF  -FLT_MAX: finite, and it overflows any sum it joins"""
import contextlib

import torch

ZERO, NAN_BITS, INF_BITS, NEG_MAX_BITS = 0x00000000, 0xFFFFFFFF, 0x7F800000, 0xFF7FFFFF
PATTERNS = (ZERO, NAN_BITS, INF_BITS, NEG_MAX_BITS)

# torch.empty_like allocates through a path of its own and never calls the Python attribute torch.empty, so no tensor is filled twice.
_REAL_EMPTY, _REAL_EMPTY_LIKE = torch.empty, torch.empty_like


class Tally:
    """What one `poisoned` block filled: `count` tensors, `nbytes` bytes of storage."""

    def __init__(self):
        self.count, self.nbytes = 0, 0


def _on(t, dev):
    dev = torch.device(dev)
    return t.device.type == dev.type and (dev.index is None or t.device.index is None or t.device.index == dev.index)


def fill_storage(t, pattern):
    """Fill every byte of t's storage with the 4-byte `pattern` (as it lies in memory, little-endian), repeated; a tail of 1..3 bytes takes
    the pattern's first bytes in order.  Returns the number of bytes filled."""
    store = t.untyped_storage()
    n = store.nbytes()
    raw = _REAL_EMPTY(0, dtype=torch.uint8, device=t.device).set_(store, 0, (n,), (1,))
    words = n // 4
    if words:
        raw[:4 * words].view(torch.int32).fill_(pattern - (1 << 32) if pattern >= (1 << 31) else pattern)
    for k in range(n - 4 * words):
        raw[4 * words + k] = (pattern >> (8 * k)) & 0xFF
    return n


@contextlib.contextmanager
def poisoned(monkeypatch, pattern, dev):
    """Within the block, torch.empty and torch.empty_like return tensors on `dev` whose whole storage holds `pattern`.  Yields the Tally
    of what was filled; both attributes are restored on exit."""
    tally = Tally()

    def wrap(real):
        def alloc(*args, **kwargs):
            t = real(*args, **kwargs)
            if torch.is_tensor(t) and _on(t, dev) and t.untyped_storage().nbytes() > 0:
                tally.nbytes += fill_storage(t, pattern)
                tally.count += 1
            return t
        return alloc

    with monkeypatch.context() as m:
        m.setattr(torch, "empty", wrap(_REAL_EMPTY))
        m.setattr(torch, "empty_like", wrap(_REAL_EMPTY_LIKE))
        yield tally


def _named(res):
    """{name: tensor} of what a closure returned: a dict, a tensor, or a (nested) sequence; None entries (an absent optional result) drop out."""
    if torch.is_tensor(res):
        return {"out": res}
    if isinstance(res, dict):
        items = list(res.items())
    else:
        items = [(str(k), v) for k, v in enumerate(res)]
    out = {}
    for n, v in items:
        if v is None:
            continue
        if torch.is_tensor(v):
            out[str(n)] = v
        else:
            out.update({"%s.%s" % (n, k): t for k, t in _named(v).items()})
    return out


def _bits(t):
    """t's elements as raw bits on the CPU: int32 for 4-byte element types, bytes for the others."""
    t = t.detach().cpu().contiguous().reshape(-1)
    if t.is_complex():
        t = torch.view_as_real(t).reshape(-1)
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.uint8)


def check(build_and_run, monkeypatch, dev, family="", shape="", reset=None, patterns=PATTERNS):
    """Run `build_and_run()` once per pattern under `poisoned` and assert, for every pattern: at least one allocation was filled (a closure
    that allocates nothing through torch.empty proves nothing); every returned floating-point element is finite; every returned tensor has
    the bits of the first (all-zero) pattern's run, no element left out.  The closure creates everything it uses -- plan or module, packed
    blob, inputs on the device, the call -- and `reset()` runs before each pattern to drop what the package caches between calls.
    Prints one row: family, shape, allocations and bytes filled in one run."""
    assert patterns[0] == ZERO, "the first pattern is the baseline"
    base, tally0 = None, None
    for pattern in patterns:
        tag = "%s %s over 0x%08X" % (family, shape, pattern)
        if reset is not None:
            reset()
        with poisoned(monkeypatch, pattern, dev) as tally:
            got = _named(build_and_run())
            if torch.device(dev).type == "cuda":
                torch.cuda.synchronize()
            got = {n: t.detach().cpu().clone() for n, t in got.items()}
        assert tally.count > 0, "%s: the closure took nothing from torch.empty on %s" % (tag, dev)
        assert got, "%s: the closure returned no tensor" % tag
        for n, t in got.items():
            if t.is_floating_point() or t.is_complex():
                assert bool(torch.isfinite(t).all()), "%s: non-finite %s" % (tag, n)
        if base is None:
            base, tally0 = got, tally
            continue
        assert set(got) == set(base), "%s: returned %s, the baseline %s" % (tag, sorted(got), sorted(base))
        for n, t in got.items():
            a, b = _bits(t), _bits(base[n])
            assert t.shape == base[n].shape and t.dtype == base[n].dtype, "%s: %s changed its shape or type" % (tag, n)
            diff = a != b
            assert not bool(diff.any()), "%s: %d of %d elements of %s differ from the zero-fill run (first at %d)" % (
                tag, int(diff.sum()), diff.numel(), n, int(diff.nonzero()[0]))
    print("fresh-memory  %-42s %-48s %4d allocations %12d bytes poisoned" % (family, shape, tally0.count, tally0.nbytes))
    return base
